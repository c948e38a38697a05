// The open-addressing table over 96-bit integer keys that the resampler (its KD-tree leaves) and the
// clusterer (its pose bins) share: the key, its hash, the table's size, and the probe that finds or
// claims a key's slot.  A slot holds the index of an item that has its key; the keys themselves stay
// in keys[item][3].  A slot is never emptied during a launch, so every item with one key walks the
// same chain to the same slot.  The key, the hash and the size are plain C++ without HIP types, host
// and device (tests/cpp/cluster_fn_check.cpp checks them through cluster/ndt2d_cluster_fn.h); the
// probe is device code.
#ifndef NDT2D_KEY_TABLE_H_
#define NDT2D_KEY_TABLE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NDT2D_KEY_TABLE_HD __host__ __device__
#else
#define NDT2D_KEY_TABLE_HD
#endif

namespace ndt2d
{
namespace particles
{

constexpr uint32_t kEmpty = 0xffffffffu;   // a slot nobody owns; "no slot"

struct Key3
{
  int32_t kx, ky, kt;
};

NDT2D_KEY_TABLE_HD inline bool same_key(const Key3 & a, const Key3 & b)
{
  return a.kx == b.kx && a.ky == b.ky && a.kt == b.kt;
}

// The slot is the hash's low bits (the table is a power of two), linear probing.
NDT2D_KEY_TABLE_HD inline uint32_t key_hash(const Key3 & k)
{
  return static_cast<uint32_t>(k.kx) * 0x9E3779B1u + static_cast<uint32_t>(k.ky) * 0x85EBCA77u +
         static_cast<uint32_t>(k.kt) * 0xC2B2AE3Du;
}

// The size of the table for n items: a power of two, at least 64 and at least 2 n.
NDT2D_KEY_TABLE_HD inline uint64_t table_size(uint64_t n)
{
  uint64_t t = 64;
  while (t < 2 * n) t <<= 1;
  return t;
}

#if defined(__HIPCC__)

__device__ __forceinline__ Key3 load_key(const int32_t * __restrict__ keys, uint64_t i)
{
  Key3 k;
  k.kx = keys[3 * i];
  k.ky = keys[3 * i + 1];
  k.kt = keys[3 * i + 2];
  return k;
}

// The slot of `key` for item `me` (keys[me] == key): the first empty slot of its chain, claimed by
// CAS, or the slot whose owner has the key.  *seen_owner is the owner this probe last saw there (`me`
// after its own claim), so a caller that keeps the SMALLEST index in a slot lowers it without a
// second load.  kEmpty when every slot holds another key (a table at most half full cannot run out).
__device__ __forceinline__ uint32_t probe_claim(const int32_t * __restrict__ keys, uint32_t * table,
                                                uint32_t mask, uint32_t me, const Key3 & key,
                                                uint32_t * seen_owner)
{
  uint32_t slot = key_hash(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe)
  {
    uint32_t owner = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (owner == kEmpty)
    {
      owner = atomicCAS(table + slot, kEmpty, me);
      if (owner == kEmpty)
      {
        *seen_owner = me;
        return slot;
      }
    }
    // whoever owns the slot, now or later, has the key of its first owner (kx first: most chains
    // part on it; then ky and kt in one load)
    const int32_t * theirs = keys + 3 * static_cast<uint64_t>(owner);
    bool same = theirs[0] == key.kx;
    if (same)
    {
      const int32_t ky = theirs[1], kt = theirs[2];
      same = (ky == key.ky) & (kt == key.kt);   // (no short circuit: both words are wanted at once)
    }
    if (same)
    {
      *seen_owner = owner;
      return slot;
    }
    slot = (slot + 1) & mask;
  }
  *seen_owner = kEmpty;
  return kEmpty;
}

#endif  // __HIPCC__

}  // namespace particles
}  // namespace ndt2d

#endif  // NDT2D_KEY_TABLE_H_
