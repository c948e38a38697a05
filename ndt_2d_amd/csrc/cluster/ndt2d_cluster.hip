// Pose clusters of a particle set (include/ndt2d_hip.h, "Pose clusters"): the particles grouped into
// connected components of occupied pose bins, the heaviest components ranked by an integer mass, and
// updateStatistics' quantities of each of them.  The arithmetic of a key is cluster/ndt2d_cluster_fn.h.
//
//   keys_kernel       one thread a particle: its key (or "left out") and its integer mass q
//   insert_kernel     the key table of particles/ndt2d_key_table.h over the keys (a power of two >= 2 n,
//                     linear probing; a slot's owner is the SMALLEST particle index with its key).
//                     The lanes of a wave that hold one key are combined first (a loop over the
//                     distinct keys: the first lane's key, a ballot of the lanes that match, a
//                     fixed butterfly of their q); one lane a key probes the table and hands its
//                     slot to the others; the group is staged in a 64-entry table of the block in
//                     LDS (integer atomics there); a block takes several tiles (at most 1,024 blocks)
//                     and sends each staged slot ONE atomicMin and two integer atomicAdds when it
//                     ends, so a converged set does not queue on one address
//   count_kernel, scan_kernel, scatter_kernel
//                     the bins in ascending owner index: the compaction of
//                     particles/ndt2d_compact.h over the flags "particle i owns its slot"; B to a
//                     device word and to the pinned block
//   neighbours_kernel one thread a bin: its 26 neighbour keys looked up in the table, their bin
//                     ranks (or -1), neighbour j of bin b at nbr[j * n + b] (a wave's loads coalesce)
//   round_kernel      one label round.  Bins are ranked by owner index, so "the smallest owner" is
//                     "the smallest bin rank" and a label is kept as a bin rank: hook (the minimum
//                     over the neighbours' labels), pointer jumping (lab <- lab[lab] until it
//                     stands still), and the old root hooked as well.  Labels only fall and always
//                     name a bin of the same component, so atomicMin in any schedule ends at the one
//                     fixed point: every bin holds the smallest rank of its component.  A round
//                     that lowered a label writes its word of the pinned block
//   mass_kernel       one thread a bin: its Q and count to its root's by integer atomics, the lanes of
//                     one root combined inside the wave first; the roots
//                     (C of them) appended to a list, a wave's at once
//   labels_kernel     every particle's label (the root's owner index)
//   select_kernel     ONE block over the roots: a sorted list of the best max_clusters per thread in LDS,
//                     then max_clusters arg-max steps over the 256 list heads (fixed trees)
//   sums_kernel, centred_kernel
//                     a block per chunk of 4,096 particles, a thread 16 of them in a fixed order;
//                     the lanes of each selected cluster present in a wave are added by a fixed
//                     butterfly, wave by wave into LDS, the block's partials to partials[chunk]
//   fold_kernel       a block per (cluster, quantity): the chunks' partials by a fixed tree
//   means_kernel, pack_kernel
//                     the means from the folded sums; the header and the records
//
// No floating-point atomic anywhere: every double sum is a fixed tree over fixed chunks of the index
// order, so two calls give the same bits.  ndt2d_cluster_launch queues everything up to the first
// label rounds; ndt2d_cluster_fetch reads the rounds' words, queues more rounds while the last one
// still lowered a label, then the masses, the selection and the statistics, and reads the block back.
//
// The clusterer is an object of its own on the public device-layer calls
// (particles/ndt2d_device_object.h): the device context has no field for it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "cluster/ndt2d_cluster_fn.h"
#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "particles/ndt2d_compact.h"
#include "particles/ndt2d_device_object.h"
#include "particles/ndt2d_key_table.h"

using namespace ndt2d::object;

namespace
{

namespace fn = ndt2d::cluster;
namespace pt = ndt2d::particles;
using pt::kEmpty;
using pt::load_key;

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxClusters = NDT2D_CLUSTER_MAX_RECORDS;
constexpr int kChunk = 4096;            // particles per block of the statistics
constexpr int kPerThread = kChunk / kBlock;
constexpr int kSums = 5;                // W, sum w x, sum w y, sum w sin, sum w cos
constexpr int kCentred = 4;             // sum w dx dx, sum w dx dy, sum w dy dy, sum w d d
constexpr int kRoundsPerRead = 4;       // label rounds queued per look at the pinned words
constexpr int kStageBits = 6;
constexpr int kStage = 1 << kStageBits; // entries of the insert's staging table in LDS
constexpr uint32_t kInsertBlocks = 1024;  // the insert's grid: a block stages several tiles before its one flush
// ctrl words
constexpr int kCtrlBins = 0, kCtrlLeftOut = 1, kCtrlClusters = 2, kCtrlFull = 3, kCtrlSelected = 4, kCtrlWords = 8;

__device__ __forceinline__ uint32_t load_u32(const uint32_t * p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 1. keys ----
__global__ void __launch_bounds__(kBlock) keys_kernel(const double * __restrict__ poses,
                                                      const double * __restrict__ weights, uint64_t n,
                                                      double uniform_w, fn::Bins bins,
                                                      int32_t * __restrict__ keys,
                                                      unsigned long long * __restrict__ q,
                                                      uint32_t * ctrl)
{
  uint32_t left_out = 0;   // of this wave (the same value in every lane)
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < n;
       base += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const uint64_t i = base + threadIdx.x;
    bool out = false;
    if (i < n)
    {
      const double w = weights != nullptr ? weights[i] : uniform_w;
      const fn::Key k = fn::key_of(poses[3 * i], poses[3 * i + 1], poses[3 * i + 2], w, bins);
      out = k.kt < 0;
      keys[3 * i] = k.kx;
      keys[3 * i + 1] = k.ky;
      keys[3 * i + 2] = k.kt;
      q[i] = out ? 0ull : static_cast<unsigned long long>(fn::mass_q(w));
    }
    left_out += static_cast<uint32_t>(__popcll(__ballot(out)));
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && left_out != 0) atomicAdd(ctrl + kCtrlLeftOut, left_out);
}

// ---- 2. the bin table ----
__global__ void __launch_bounds__(kBlock) insert_kernel(const int32_t * __restrict__ keys,
                                                        const unsigned long long * __restrict__ q,
                                                        uint64_t n, uint32_t * owner,
                                                        unsigned long long * slot_q, uint32_t * slot_count,
                                                        uint32_t mask, uint32_t * __restrict__ bin_of,
                                                        uint32_t * ctrl)
{
  // the block's staging table: the groups of its waves are added here first (LDS integer atomics)
  // and go to the slots once, when the block ends; a group that finds no entry goes there directly
  __shared__ uint32_t st_slot[kStage];
  __shared__ uint32_t st_min[kStage];
  __shared__ uint32_t st_count[kStage];
  __shared__ unsigned long long st_q[kStage];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  if (threadIdx.x < kStage)
  {
    st_slot[threadIdx.x] = kEmpty;
    st_min[threadIdx.x] = kEmpty;
    st_count[threadIdx.x] = 0u;
    st_q[threadIdx.x] = 0ull;
  }
  __syncthreads();
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < n;
       base += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const uint64_t i = base + threadIdx.x;
    const uint32_t me = static_cast<uint32_t>(i);
    fn::Key k;
    k.kx = 0;
    k.ky = 0;
    k.kt = -1;
    unsigned long long mine = 0;
    if (i < n)
    {
      k = load_key(keys, i);
      if (k.kt >= 0) mine = q[i];
    }
    // The lanes of this wave grouped by key, every lane walking the same loop: a group's first lane
    // (its smallest particle index) becomes its leader and keeps the group's q and size.
    bool leader = false;
    uint32_t leader_lane = lane;
    unsigned long long group_q = 0;
    uint32_t group_size = 0;
    unsigned long long todo = __ballot(k.kt >= 0);
    while (todo != 0)
    {
      const int first = __ffsll(static_cast<long long>(todo)) - 1;
      fn::Key f;
      f.kx = __shfl(k.kx, first, kWave);
      f.ky = __shfl(k.ky, first, kWave);
      f.kt = __shfl(k.kt, first, kWave);
      const bool member = fn::same_key(k, f);   // (f.kt >= 0: the lanes left out do not match)
      const unsigned long long group = __ballot(member);
      const uint32_t members = static_cast<uint32_t>(__popcll(group));
      unsigned long long sum = mine;
      if (members > 1)
      {
        sum = member ? mine : 0ull;
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
      }
      if (member) leader_lane = static_cast<uint32_t>(first);
      if (static_cast<int>(lane) == first)
      {
        leader = true;
        group_q = sum;
        group_size = members;
      }
      todo &= ~group;
    }
    // the leaders probe, one lane a distinct key: a converged set sends a wave's one request to the
    // slot's address where a lane each would queue sixty-four
    uint32_t found = kEmpty;
    if (leader)
    {
      uint32_t seen;   // (the owner is lowered once, from the staging table)
      found = pt::probe_claim(keys, owner, mask, me, k, &seen);
      if (found == kEmpty) atomicOr(ctrl + kCtrlFull, 1u);   // (a table at most half full cannot run out)
    }
    found = __shfl(found, leader_lane, kWave);
    if (i < n) bin_of[i] = k.kt >= 0 ? found : kEmpty;
    if (leader && found != kEmpty)
    {
      const uint32_t s = found;
      bool staged = false;
      uint32_t e = (s * 0x9E3779B1u) >> (32 - kStageBits);
      for (int probe = 0; probe < 4 && !staged; ++probe)
      {
        const uint32_t tag = atomicCAS(st_slot + e, kEmpty, s);
        if (tag == kEmpty || tag == s)
        {
          atomicMin(st_min + e, me);
          atomicAdd(st_q + e, group_q);
          atomicAdd(st_count + e, group_size);
          staged = true;
        }
        e = (e + 1) & (kStage - 1);
      }
      if (!staged)
      {
        if (me < load_u32(owner + s)) atomicMin(owner + s, me);
        if (group_q != 0) atomicAdd(slot_q + s, group_q);
        atomicAdd(slot_count + s, group_size);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kStage && st_slot[threadIdx.x] != kEmpty)
  {
    const uint32_t s = st_slot[threadIdx.x];
    if (st_min[threadIdx.x] < load_u32(owner + s)) atomicMin(owner + s, st_min[threadIdx.x]);
    if (st_q[threadIdx.x] != 0) atomicAdd(slot_q + s, st_q[threadIdx.x]);
    atomicAdd(slot_count + s, st_count[threadIdx.x]);
  }
}

// ---- 3. the bin list ----
__device__ __forceinline__ bool owns_bin(const uint32_t * __restrict__ owner,
                                         const uint32_t * __restrict__ bin_of, uint64_t n, uint64_t i)
{
  if (i >= n) return false;
  const uint32_t s = bin_of[i];
  return s != kEmpty && owner[s] == static_cast<uint32_t>(i);
}

__global__ void __launch_bounds__(kBlock) count_kernel(const uint32_t * __restrict__ owner,
                                                       const uint32_t * __restrict__ bin_of, uint64_t n,
                                                       uint32_t * __restrict__ sums)
{
  pt::tile_count(owns_bin(owner, bin_of, n, static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x), sums);
}

// sums[b] -> bins in the tiles before b; the total B to ctrl and to the pinned block
__global__ void __launch_bounds__(kBlock) scan_kernel(uint32_t * sums, uint32_t n_tiles, uint32_t * ctrl,
                                                      uint32_t * host_bins)
{
  const uint32_t total = pt::scan_tile_sums(sums, n_tiles);
  if (threadIdx.x == kBlock - 1)
  {
    ctrl[kCtrlBins] = total;
    // the pinned word, written through at system scope (a vector store)
    __hip_atomic_store(host_bins, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ void __launch_bounds__(kBlock) scatter_kernel(const uint32_t * __restrict__ owner,
                                                         const uint32_t * __restrict__ bin_of, uint64_t n,
                                                         const uint32_t * __restrict__ sums,
                                                         uint32_t * __restrict__ bin_slot,
                                                         uint32_t * __restrict__ bin_owner,
                                                         uint32_t * __restrict__ rank_of_slot,
                                                         uint32_t * __restrict__ lab,
                                                         unsigned long long * __restrict__ root_q,
                                                         uint32_t * __restrict__ root_count)
{
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool flag = owns_bin(owner, bin_of, n, i);
  const uint32_t rank = pt::tile_rank(flag, sums);
  if (!flag) return;
  if (rank >= n) return;   // (a bin has an owner: B <= n; the test keeps a stray count inside the arrays)
  const uint32_t s = bin_of[i];
  bin_slot[rank] = s;
  bin_owner[rank] = static_cast<uint32_t>(i);
  rank_of_slot[s] = rank;
  lab[rank] = rank;
  root_q[rank] = 0ull;
  root_count[rank] = 0u;
}

__global__ void __launch_bounds__(kBlock) neighbours_kernel(const int32_t * __restrict__ keys,
                                                            const uint32_t * __restrict__ owner,
                                                            const uint32_t * __restrict__ rank_of_slot,
                                                            const uint32_t * __restrict__ bin_owner,
                                                            const uint32_t * __restrict__ ctrl, uint32_t mask,
                                                            int32_t n_theta, uint64_t n,
                                                            int32_t * __restrict__ nbr)
{
  const uint64_t n_bins = ctrl[kCtrlBins] < n ? ctrl[kCtrlBins] : n;
  for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; b < n_bins;
       b += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const fn::Key k = load_key(keys, bin_owner[b]);
    for (int j = 0; j < fn::kNeighbours; ++j)
    {
      const fn::Key want = fn::neighbour(k, j, n_theta);
      int32_t rank = -1;
      uint32_t slot = fn::key_hash(want) & mask;
      for (uint32_t probe = 0; probe <= mask; ++probe)
      {
        const uint32_t o = owner[slot];
        if (o == kEmpty) break;
        if (fn::same_key(load_key(keys, o), want))
        {
          rank = static_cast<int32_t>(rank_of_slot[slot]);
          break;
        }
        slot = (slot + 1) & mask;
      }
      nbr[static_cast<uint64_t>(j) * n + b] = rank;
    }
  }
}

// ---- 4. the labels ----
__global__ void __launch_bounds__(kBlock) round_kernel(const int32_t * __restrict__ nbr, uint32_t * lab,
                                                       const uint32_t * __restrict__ ctrl, uint64_t n,
                                                       uint32_t * host_changed)
{
  const uint64_t n_bins = ctrl[kCtrlBins] < n ? ctrl[kCtrlBins] : n;
  bool changed = false;
  for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; b < n_bins;
       b += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const uint32_t old = load_u32(lab + b);
    uint32_t m = old;
    for (int j = 0; j < fn::kNeighbours; ++j)
    {
      const int32_t r = nbr[static_cast<uint64_t>(j) * n + b];
      if (r >= 0)
      {
        const uint32_t l = load_u32(lab + r);
        m = l < m ? l : m;
      }
    }
    // pointer jumping: labels only fall and lab[x] <= x, so the walk ends
    for (uint32_t p = load_u32(lab + m); p < m; p = load_u32(lab + m)) m = p;
    if (m < old)
    {
      atomicMin(lab + b, m);
      if (m < load_u32(lab + old)) atomicMin(lab + old, m);   // the old root joins as well
      changed = true;
    }
  }
  if (__ballot(changed) != 0 && (threadIdx.x & (kWave - 1)) == 0)
  {
    __hip_atomic_store(host_changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- 5. the clusters' masses ----
__global__ void __launch_bounds__(kBlock) mass_kernel(const uint32_t * __restrict__ lab,
                                                      const uint32_t * __restrict__ bin_slot,
                                                      const unsigned long long * __restrict__ slot_q,
                                                      const uint32_t * __restrict__ slot_count,
                                                      unsigned long long * root_q, uint32_t * root_count,
                                                      uint32_t * __restrict__ root_list, uint32_t * ctrl,
                                                      uint64_t n)
{
  const uint64_t n_bins = ctrl[kCtrlBins] < n ? ctrl[kCtrlBins] : n;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < n_bins;
       base += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const uint64_t b = base + threadIdx.x;
    bool root = false;
    uint32_t r = kEmpty;
    unsigned long long mass = 0;
    uint32_t count = 0;
    if (b < n_bins)
    {
      r = lab[b];
      const uint32_t s = bin_slot[b];
      root = r == static_cast<uint32_t>(b);
      mass = slot_q[s];
      count = slot_count[s];
    }
    // one atomic of each kind per distinct root of this wave (a set seeded over one connected free
    // space has nearly every bin under one root); every lane walks the same loop
    unsigned long long todo = __ballot(r != kEmpty);
    while (todo != 0)
    {
      const int first = __ffsll(static_cast<long long>(todo)) - 1;
      const uint32_t want = __shfl(r, first, kWave);
      const bool member = r == want;
      const unsigned long long group = __ballot(member);
      unsigned long long sum = mass;
      uint32_t size = count;
      if (__popcll(group) > 1)
      {
        sum = member ? mass : 0ull;
        size = member ? count : 0u;
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1)
        {
          sum += __shfl_xor(sum, off, kWave);
          size += __shfl_xor(size, off, kWave);
        }
      }
      if (static_cast<int>(lane) == first)
      {
        if (sum != 0) atomicAdd(root_q + want, sum);
        atomicAdd(root_count + want, size);
      }
      todo &= ~group;
    }
    // the roots into a list, a wave's at once: its order depends on the schedule, what is selected
    // from it does not (the rank is a total order)
    const unsigned long long ballot = __ballot(root);
    if (ballot != 0)
    {
      const int first = __ffsll(static_cast<long long>(ballot)) - 1;
      uint32_t at = 0;
      if (static_cast<int>(lane) == first) at = atomicAdd(ctrl + kCtrlClusters, static_cast<uint32_t>(__popcll(ballot)));
      at = __shfl(at, first, kWave) + static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
      if (root && at < n) root_list[at] = static_cast<uint32_t>(b);
    }
  }
}

// every particle's label: the owner index of its bin's root
__global__ void __launch_bounds__(kBlock) labels_kernel(const uint32_t * __restrict__ bin_of,
                                                        const uint32_t * __restrict__ rank_of_slot,
                                                        const uint32_t * __restrict__ lab,
                                                        const uint32_t * __restrict__ bin_owner, uint64_t n,
                                                        uint32_t * __restrict__ labels)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const uint32_t s = bin_of[i];
    labels[i] = s == kEmpty ? fn::kLeftOut : bin_owner[lab[rank_of_slot[s]]];
  }
}

// ---- 6. the selection ----
struct Selected
{
  uint32_t label[kMaxClusters];
  uint32_t count[kMaxClusters];
  unsigned long long q[kMaxClusters];
};

// One block.  Each thread keeps the best `want` roots of its strided share as a sorted list in LDS
// (list position p of thread t at [p][t]); then `want` times: the best head over the 256 lists by a
// fixed tree, and the winner's list moves on.  The order is total, so the list is the list.
__global__ void __launch_bounds__(kBlock) select_kernel(const uint32_t * __restrict__ root_list,
                                                        const uint32_t * __restrict__ bin_owner,
                                                        const unsigned long long * __restrict__ root_q,
                                                        const uint32_t * __restrict__ root_count,
                                                        uint32_t * ctrl, uint64_t n, int want,
                                                        Selected * __restrict__ out)
{
  __shared__ unsigned long long list_q[kMaxClusters][kBlock];
  __shared__ uint32_t list_rank[kMaxClusters][kBlock];
  __shared__ unsigned long long best_q[kBlock];
  __shared__ uint32_t best_rank[kBlock];
  __shared__ uint32_t best_thread[kBlock];
  const uint32_t t = threadIdx.x;
  const uint64_t n_roots = ctrl[kCtrlClusters] < n ? ctrl[kCtrlClusters] : n;
  for (int p = 0; p < want; ++p)
  {
    list_q[p][t] = 0ull;
    list_rank[p][t] = kEmpty;
  }
  // (a root's rank orders as its label does: bins are ranked by owner index)
  for (uint64_t k = t; k < n_roots; k += kBlock)
  {
    const uint32_t b = root_list[k];
    unsigned long long cq = root_q[b];
    uint32_t cr = b;
    if (!fn::ranks_before(cq, cr, list_q[want - 1][t], list_rank[want - 1][t])) continue;
    for (int p = 0; p < want; ++p)
    {
      const unsigned long long hq = list_q[p][t];
      const uint32_t hr = list_rank[p][t];
      if (fn::ranks_before(cq, cr, hq, hr))
      {
        list_q[p][t] = cq;
        list_rank[p][t] = cr;
        cq = hq;
        cr = hr;
      }
    }
  }
  int head = 0;
  uint32_t n_selected = 0;
  for (int k = 0; k < want; ++k)
  {
    best_q[t] = head < want ? list_q[head][t] : 0ull;
    best_rank[t] = head < want ? list_rank[head][t] : kEmpty;
    best_thread[t] = t;
    __syncthreads();
    for (uint32_t d = kBlock / 2; d > 0; d >>= 1)
    {
      if (t < d && fn::ranks_before(best_q[t + d], best_rank[t + d], best_q[t], best_rank[t]))
      {
        best_q[t] = best_q[t + d];
        best_rank[t] = best_rank[t + d];
        best_thread[t] = best_thread[t + d];
      }
      __syncthreads();
    }
    const uint32_t rank = best_rank[0];
    const uint32_t winner = best_thread[0];
    __syncthreads();
    if (rank == kEmpty) break;   // fewer clusters than records (the same decision in every thread)
    if (t == winner) ++head;
    if (t == 0)
    {
      out->label[k] = bin_owner[rank];
      out->count[k] = root_count[rank];
      out->q[k] = root_q[rank];
    }
    ++n_selected;
  }
  if (t == 0)
  {
    for (int k = static_cast<int>(n_selected); k < kMaxClusters; ++k)
    {
      out->label[k] = kEmpty;
      out->count[k] = 0u;
      out->q[k] = 0ull;
    }
    ctrl[kCtrlSelected] = n_selected;
  }
}

// ---- 7. the statistics ----
struct Means
{
  double w[kMaxClusters + 1];   // [kMaxClusters]: W_total
  double mx[kMaxClusters], my[kMaxClusters], mt[kMaxClusters];
};

// The members of cluster c among this wave's lanes, their `count` values added by a fixed butterfly
// into acc[c][0 .. count) by lane 0.  `member` is uniform in nothing; the ballot makes the skip so.
template <int kValues>
__device__ __forceinline__ void add_members(bool member, const double (&v)[kValues], double * acc, uint32_t lane)
{
  if (__ballot(member) == 0) return;
#pragma unroll
  for (int j = 0; j < kValues; ++j)
  {
    double s = member ? v[j] : 0.0;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    if (lane == 0) acc[j] += s;
  }
}

// the waves' accumulators added in wave order into partials[chunk][slot][value]
template <int kValues, int kSlots>
__device__ __forceinline__ void store_partials(const double (*acc)[kSlots][kValues], double * __restrict__ partials)
{
  for (int e = threadIdx.x; e < kSlots * kValues; e += kBlock)
  {
    const int c = e / kValues, j = e - c * kValues;
    double s = acc[0][c][j];
    for (int w = 1; w < kWaves; ++w) s += acc[w][c][j];
    partials[(static_cast<uint64_t>(blockIdx.x) * kSlots + c) * kValues + j] = s;
  }
}

__device__ __forceinline__ int selected_index(const uint32_t * sel, int n_sel, uint32_t label)
{
  int c = -1;
  for (int k = 0; k < n_sel; ++k) c = sel[k] == label ? k : c;
  return c;
}

// pass 1: W, sum w x, sum w y, sum w sin, sum w cos of each selected cluster; slot kMaxClusters
// holds, in value 0, the weight of every particle that is not left out (W_total)
__global__ void __launch_bounds__(kBlock) sums_kernel(const double * __restrict__ poses,
                                                      const double * __restrict__ weights, uint64_t n,
                                                      double uniform_w, const uint32_t * __restrict__ labels,
                                                      const Selected * __restrict__ selected,
                                                      const uint32_t * __restrict__ ctrl,
                                                      double * __restrict__ partials)
{
  __shared__ double acc[kWaves][kMaxClusters + 1][kSums];
  __shared__ uint32_t sel[kMaxClusters];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int n_sel = static_cast<int>(ctrl[kCtrlSelected]);
  if (threadIdx.x < kMaxClusters) sel[threadIdx.x] = selected->label[threadIdx.x];
  for (int e = threadIdx.x; e < kWaves * (kMaxClusters + 1) * kSums; e += kBlock) (&acc[0][0][0])[e] = 0.0;
  __syncthreads();
  for (int k = 0; k < kPerThread; ++k)
  {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kChunk + static_cast<uint64_t>(k) * kBlock + threadIdx.x;
    int c = -1;
    bool counted = false;
    double v[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n)
    {
      const uint32_t label = labels[i];
      counted = label != fn::kLeftOut;
      if (counted)
      {
        v[0] = weights != nullptr ? weights[i] : uniform_w;
        c = selected_index(sel, n_sel, label);
      }
      if (c >= 0)
      {
        const double th = poses[3 * i + 2];
        v[1] = v[0] * poses[3 * i];
        v[2] = v[0] * poses[3 * i + 1];
        v[3] = v[0] * sin(th);
        v[4] = v[0] * cos(th);
      }
    }
    for (int s = 0; s < n_sel; ++s) add_members<kSums>(c == s, v, acc[wave][s], lane);
    const double total[1] = {v[0]};
    add_members<1>(counted, total, acc[wave][kMaxClusters], lane);
  }
  __syncthreads();
  store_partials<kSums, kMaxClusters + 1>(acc, partials);
}

// pass 2: the centred second moments and the squared angular distance round the means
__global__ void __launch_bounds__(kBlock) centred_kernel(const double * __restrict__ poses,
                                                         const double * __restrict__ weights, uint64_t n,
                                                         double uniform_w, const uint32_t * __restrict__ labels,
                                                         const Selected * __restrict__ selected,
                                                         const uint32_t * __restrict__ ctrl,
                                                         const Means * __restrict__ means,
                                                         double * __restrict__ partials)
{
  __shared__ double acc[kWaves][kMaxClusters][kCentred];
  __shared__ uint32_t sel[kMaxClusters];
  __shared__ double mx[kMaxClusters], my[kMaxClusters], mt[kMaxClusters];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int n_sel = static_cast<int>(ctrl[kCtrlSelected]);
  if (threadIdx.x < kMaxClusters)
  {
    sel[threadIdx.x] = selected->label[threadIdx.x];
    mx[threadIdx.x] = means->mx[threadIdx.x];
    my[threadIdx.x] = means->my[threadIdx.x];
    mt[threadIdx.x] = means->mt[threadIdx.x];
  }
  for (int e = threadIdx.x; e < kWaves * kMaxClusters * kCentred; e += kBlock) (&acc[0][0][0])[e] = 0.0;
  __syncthreads();
  for (int k = 0; k < kPerThread; ++k)
  {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kChunk + static_cast<uint64_t>(k) * kBlock + threadIdx.x;
    int c = -1;
    double v[kCentred] = {0.0, 0.0, 0.0, 0.0};
    if (i < n)
    {
      const uint32_t label = labels[i];
      if (label != fn::kLeftOut) c = selected_index(sel, n_sel, label);
      if (c >= 0)
      {
        const double w = weights != nullptr ? weights[i] : uniform_w;
        const double dx = poses[3 * i] - mx[c];
        const double dy = poses[3 * i + 1] - my[c];
        const double d = fn::normalise_angle(poses[3 * i + 2] - mt[c]);
        v[0] = w * dx * dx;
        v[1] = w * dx * dy;
        v[2] = w * dy * dy;
        v[3] = w * d * d;
      }
    }
    for (int s = 0; s < n_sel; ++s) add_members<kCentred>(c == s, v, acc[wave][s], lane);
  }
  __syncthreads();
  store_partials<kCentred, kMaxClusters>(acc, partials);
}

// block e = (slot, value): partials[chunk][e] over the chunks by a strided share per thread, the
// waves' butterflies and the block's fixed sum
__global__ void __launch_bounds__(kBlock) fold_kernel(const double * __restrict__ partials, uint32_t n_chunks,
                                                      uint32_t n_values, double * __restrict__ out)
{
  __shared__ double sh[kWaves];
  double total = 0.0;
  for (uint32_t b = threadIdx.x; b < n_chunks; b += kBlock) total += partials[static_cast<uint64_t>(b) * n_values + blockIdx.x];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((sh[0] + sh[1]) + (sh[2] + sh[3]));
}

__global__ void __launch_bounds__(kWave) means_kernel(const double * __restrict__ sums, const uint32_t * __restrict__ ctrl,
                                                      Means * __restrict__ means)
{
  const int c = threadIdx.x;
  if (c > kMaxClusters) return;
  const double w = sums[c * kSums];
  means->w[c] = w;
  if (c == kMaxClusters) return;
  const bool live = c < static_cast<int>(ctrl[kCtrlSelected]);
  means->mx[c] = live ? sums[c * kSums + 1] / w : 0.0;
  means->my[c] = live ? sums[c * kSums + 2] / w : 0.0;
  means->mt[c] = live ? atan2(sums[c * kSums + 3], sums[c * kSums + 4]) : 0.0;
}

struct Packed
{
  ndt2d_cluster_header header;
  ndt2d_cluster_record records[kMaxClusters];
  uint32_t table_full;   // a particle found no slot (cannot happen in a table at most half full)
};

__global__ void __launch_bounds__(kWave) pack_kernel(const uint32_t * __restrict__ ctrl, uint64_t n,
                                                     const Selected * __restrict__ selected,
                                                     const Means * __restrict__ means,
                                                     const double * __restrict__ centred, Packed * __restrict__ out)
{
  const int c = threadIdx.x;
  if (c == 0)
  {
    out->header.n = n;
    out->header.n_left_out = ctrl[kCtrlLeftOut];
    out->header.n_bins = ctrl[kCtrlBins];
    out->header.n_clusters = ctrl[kCtrlClusters];
    out->header.rounds = 0;   // the host's count
    out->header.w_total = means->w[kMaxClusters];
    out->table_full = ctrl[kCtrlFull];
  }
  if (c >= kMaxClusters) return;
  const bool live = c < static_cast<int>(ctrl[kCtrlSelected]);
  ndt2d_cluster_record r;
  const double w = means->w[c];
  r.label = live ? selected->label[c] : fn::kLeftOut;
  r.count = live ? selected->count[c] : 0u;
  r.mass = live ? static_cast<double>(selected->q[c]) * fn::kInv40 : 0.0;
  r.weight = live ? w : 0.0;
  r.mean_x = live ? means->mx[c] : 0.0;
  r.mean_y = live ? means->my[c] : 0.0;
  r.mean_theta = live ? means->mt[c] : 0.0;
  r.cxx = live ? centred[c * kCentred] / w : 0.0;
  r.cxy = live ? centred[c * kCentred + 1] / w : 0.0;
  r.cyy = live ? centred[c * kCentred + 2] / w : 0.0;
  r.var_theta = live ? centred[c * kCentred + 3] / w : 0.0;
  out->records[c] = r;
}

// the pinned block: the bins, the label rounds' words, the results
struct HostBlock
{
  uint32_t bins;
  uint32_t changed[kRoundsPerRead];
  Packed packed;
};

enum Phase { kPhaseTable = 0, kPhaseBins, kPhaseLabels, kPhaseSelect, kPhaseStats, kPhases };

}  // namespace

struct ndt2d_clusterer : DeviceObject
{
  size_t n_cap = 0;

  fn::Bins bins{0.5, 0.5, 24};
  int max_clusters = 8;

  void * workspace = nullptr;
  int32_t * keys = nullptr;              // [n_cap][3]
  unsigned long long * q = nullptr;      // [n_cap]
  uint32_t * bin_of = nullptr;           // [n_cap] a particle's slot
  uint32_t * labels = nullptr;           // [n_cap] a particle's label
  uint32_t * owner = nullptr;            // [table]
  unsigned long long * slot_q = nullptr; // [table]
  uint32_t * slot_count = nullptr;       // [table]
  uint32_t * rank_of_slot = nullptr;     // [table]
  uint32_t * sums = nullptr;             // [tiles]
  uint32_t * bin_slot = nullptr;         // [n_cap]
  uint32_t * bin_owner = nullptr;        // [n_cap]
  uint32_t * lab = nullptr;              // [n_cap] a bin's label, as a bin rank
  unsigned long long * root_q = nullptr; // [n_cap]
  uint32_t * root_count = nullptr;       // [n_cap]
  uint32_t * root_list = nullptr;        // [n_cap] the roots' bin ranks, in no particular order
  int32_t * nbr = nullptr;               // [26][n] of the call: neighbour j of bin b at [j * n + b]
  double * partials = nullptr;           // [chunks][17][5]
  double * folded = nullptr;             // [17 * 5] and [16 * 4]
  Means * means = nullptr;
  Selected * selected = nullptr;
  Packed * packed = nullptr;
  uint32_t * ctrl = nullptr;             // [kCtrlWords]
  Pinned<HostBlock> pinned;

  // the launch a fetch completes
  bool launched = false, fetched = false;
  hipStream_t stream = nullptr;
  const double * d_poses = nullptr;
  const double * d_weights = nullptr;
  uint64_t n = 0;
  Packed result;

  bool timing = false, timed = false;
  hipEvent_t ev[kPhases + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

namespace
{

void release(ndt2d_clusterer * c)
{
  for (hipEvent_t e : c->ev)
  {
    if (e != nullptr) (void)hipEventDestroy(e);
  }
  if (c->workspace != nullptr) (void)ndt2d_device_free(c->h, c->workspace);
  pinned_free(c, &c->pinned);
  delete c;
}

uint32_t chunks_of(uint64_t n) { return static_cast<uint32_t>((n + kChunk - 1) / kChunk); }

// kRoundsPerRead more label rounds, each with its own word of the pinned block
int queue_rounds(ndt2d_clusterer * c)
{
  for (int r = 0; r < kRoundsPerRead; ++r) __atomic_store_n(&c->pinned.host->changed[r], 0u, __ATOMIC_RELEASE);
  for (int r = 0; r < kRoundsPerRead; ++r)
  {
    hipLaunchKernelGGL(round_kernel, dim3(stride_blocks(c->n, kBlock)), dim3(kBlock), 0, c->stream, c->nbr, c->lab,
                       c->ctrl, c->n, &c->pinned.dev->changed[r]);
    NDT2D_OBJ_HIP(c, hipGetLastError());
  }
  return NDT2D_OK;
}

// after the labels stand: masses, particle labels, selection, statistics, the block to the host
int queue_rest(ndt2d_clusterer * c)
{
  hipStream_t s = c->stream;
  const uint64_t n = c->n;
  const uint32_t blocks = stride_blocks(n, kBlock), chunks = chunks_of(n);
  const double uniform_w = 1.0 / static_cast<double>(n);
  hipLaunchKernelGGL(mass_kernel, dim3(blocks), dim3(kBlock), 0, s, c->lab, c->bin_slot, c->slot_q,
                     c->slot_count, c->root_q, c->root_count, c->root_list, c->ctrl, n);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(labels_kernel, dim3(blocks), dim3(kBlock), 0, s, c->bin_of, c->rank_of_slot, c->lab,
                     c->bin_owner, n, c->labels);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(select_kernel, dim3(1), dim3(kBlock), 0, s, c->root_list, c->bin_owner, c->root_q,
                     c->root_count, c->ctrl, n, c->max_clusters, c->selected);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->ev[kPhaseStats], s));
  hipLaunchKernelGGL(sums_kernel, dim3(chunks), dim3(kBlock), 0, s, c->d_poses, c->d_weights, n, uniform_w,
                     c->labels, c->selected, c->ctrl, c->partials);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(fold_kernel, dim3((kMaxClusters + 1) * kSums), dim3(kBlock), 0, s, c->partials, chunks,
                     static_cast<uint32_t>((kMaxClusters + 1) * kSums), c->folded);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(means_kernel, dim3(1), dim3(kWave), 0, s, c->folded, c->ctrl, c->means);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(centred_kernel, dim3(chunks), dim3(kBlock), 0, s, c->d_poses, c->d_weights, n, uniform_w,
                     c->labels, c->selected, c->ctrl, c->means, c->partials);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  double * centred = c->folded + (kMaxClusters + 1) * kSums;
  hipLaunchKernelGGL(fold_kernel, dim3(kMaxClusters * kCentred), dim3(kBlock), 0, s, c->partials, chunks,
                     static_cast<uint32_t>(kMaxClusters * kCentred), centred);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(pack_kernel, dim3(1), dim3(kWave), 0, s, c->ctrl, n, c->selected, c->means, centred,
                     c->packed);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  NDT2D_OBJ_HIP(c, hipMemcpyAsync(&c->pinned.host->packed, c->packed, sizeof(Packed), hipMemcpyDeviceToHost, s));
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->ev[kPhases], s));
  return NDT2D_OK;
}

}  // namespace

extern "C" {

int ndt2d_cluster_create(ndt2d_handle h, size_t max_particles, ndt2d_clusterer ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  // (2^23 particles of weight <= 1 keep a cluster's Q below 2^63)
  if (h == nullptr || max_particles == 0 || max_particles > (1ull << 23)) return NDT2D_ERR_INVALID;
  ndt2d_clusterer * c = new ndt2d_clusterer();
  c->h = h;
  c->device = ndt2d_device_id(h);
  c->n_cap = max_particles;
  const size_t m = max_particles;
  const size_t table = static_cast<size_t>(fn::table_size(m));
  const size_t tiles = (m + kBlock - 1) / kBlock;
  const size_t n_partials = static_cast<size_t>(chunks_of(m)) * (kMaxClusters + 1) * kSums;
  const size_t n_folded = (kMaxClusters + 1) * kSums + kMaxClusters * kCentred;
  const size_t bytes =
    align_up(3 * m * sizeof(int32_t)) + align_up(m * sizeof(unsigned long long)) + 2 * align_up(m * sizeof(uint32_t)) +
    3 * align_up(table * sizeof(uint32_t)) + align_up(table * sizeof(unsigned long long)) +
    align_up(tiles * sizeof(uint32_t)) + 5 * align_up(m * sizeof(uint32_t)) + align_up(m * sizeof(unsigned long long)) +
    align_up(static_cast<size_t>(fn::kNeighbours) * m * sizeof(int32_t)) + align_up(n_partials * sizeof(double)) +
    align_up(n_folded * sizeof(double)) + align_up(sizeof(Means)) + align_up(sizeof(Selected)) +
    align_up(sizeof(Packed)) + align_up(kCtrlWords * sizeof(uint32_t));
  int rc = ndt2d_device_alloc(h, bytes, &c->workspace);
  if (rc == NDT2D_OK) rc = pinned_alloc(c, &c->pinned);
  if (rc != NDT2D_OK)
  {
    release(c);
    return rc;
  }
  char * p = static_cast<char *>(c->workspace);
  c->keys = carve<int32_t>(&p, 3 * m);
  c->q = carve<unsigned long long>(&p, m);
  c->bin_of = carve<uint32_t>(&p, m);
  c->labels = carve<uint32_t>(&p, m);
  c->owner = carve<uint32_t>(&p, table);
  c->slot_count = carve<uint32_t>(&p, table);
  c->rank_of_slot = carve<uint32_t>(&p, table);
  c->slot_q = carve<unsigned long long>(&p, table);
  c->sums = carve<uint32_t>(&p, tiles);
  c->bin_slot = carve<uint32_t>(&p, m);
  c->bin_owner = carve<uint32_t>(&p, m);
  c->lab = carve<uint32_t>(&p, m);
  c->root_count = carve<uint32_t>(&p, m);
  c->root_list = carve<uint32_t>(&p, m);
  c->root_q = carve<unsigned long long>(&p, m);
  c->nbr = carve<int32_t>(&p, static_cast<size_t>(fn::kNeighbours) * m);
  c->partials = carve<double>(&p, n_partials);
  c->folded = carve<double>(&p, n_folded);
  c->means = carve<Means>(&p, 1);
  c->selected = carve<Selected>(&p, 1);
  c->packed = carve<Packed>(&p, 1);
  c->ctrl = carve<uint32_t>(&p, kCtrlWords);
  std::memset(c->pinned.host, 0, sizeof(HostBlock));
  std::memset(&c->result, 0, sizeof(Packed));
  hipError_t e = hipSuccess;
  for (hipEvent_t & ev : c->ev)
  {
    if (e == hipSuccess) e = hipEventCreate(&ev);
  }
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    release(c);
    return NDT2D_ERR_HIP;
  }
  *out = c;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_cluster_destroy(ndt2d_clusterer * c)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (c->stream != nullptr) (void)hipStreamSynchronize(c->stream);
  release(c);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_cluster_last_error(ndt2d_clusterer * c) { return c != nullptr ? c->err.c_str() : ""; }

int ndt2d_cluster_set_bins(ndt2d_clusterer * c, double cell_x, double cell_y, int n_theta)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (!std::isfinite(cell_x) || !std::isfinite(cell_y) || !(cell_x > 0.0) || !(cell_y > 0.0))
  {
    return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_set_bins: a cell size is not finite and positive");
  }
  if (n_theta < 1) return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_set_bins: n_theta is below 1");
  c->bins = fn::Bins{cell_x, cell_y, n_theta};
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_cluster_set_max_clusters(ndt2d_clusterer * c, int max_clusters)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (max_clusters < 1 || max_clusters > kMaxClusters)
  {
    return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_set_max_clusters: not in 1 .. 16");
  }
  c->max_clusters = max_clusters;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_cluster_set_timing(ndt2d_clusterer * c, int enabled)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  c->timing = enabled != 0;
  if (!c->timing) c->timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_cluster_last_ms(ndt2d_clusterer * c, float * ms5)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (ms5 == nullptr) return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_last_ms: null argument");
  if (!c->timed) return fail(c, NDT2D_ERR_STATE, "ndt2d_cluster_last_ms: no timed call has been fetched");
  NDT2D_OBJ_HIP(c, hipSetDevice(c->device));
  for (int p = 0; p < kPhases; ++p) NDT2D_OBJ_HIP(c, hipEventElapsedTime(ms5 + p, c->ev[p], c->ev[p + 1]));
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_cluster_launch(ndt2d_clusterer * c, const double * d_poses_xyt, const double * d_weights, size_t n)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (n > c->n_cap) return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_launch: more particles than the clusterer was made for");
  if (n > 0 && d_poses_xyt == nullptr) return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_launch: null poses");
  NDT2D_OBJ_HIP(c, hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(ndt2d_get_stream(c->h));
  // work queued on a stream the caller has since replaced finishes first
  if (c->stream != nullptr && c->stream != s) NDT2D_OBJ_HIP(c, hipStreamSynchronize(c->stream));
  c->stream = s;
  c->launched = false;
  c->fetched = false;
  c->timed = false;
  c->d_poses = d_poses_xyt;
  c->d_weights = d_weights;
  c->n = n;
  if (n == 0)
  {
    c->launched = true;
    return NDT2D_OK;
  }
  const uint64_t n64 = n;
  const uint64_t table = fn::table_size(n64);
  const uint32_t mask = static_cast<uint32_t>(table - 1);
  const uint32_t blocks = stride_blocks(n64, kBlock);
  const uint32_t tiles = static_cast<uint32_t>((n64 + kBlock - 1) / kBlock);
  NDT2D_OBJ_HIP(c, hipMemsetAsync(c->owner, 0xff, table * sizeof(uint32_t), s));
  NDT2D_OBJ_HIP(c, hipMemsetAsync(c->slot_count, 0, table * sizeof(uint32_t), s));
  NDT2D_OBJ_HIP(c, hipMemsetAsync(c->slot_q, 0, table * sizeof(unsigned long long), s));
  NDT2D_OBJ_HIP(c, hipMemsetAsync(c->ctrl, 0, kCtrlWords * sizeof(uint32_t), s));
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->ev[kPhaseTable], s));
  hipLaunchKernelGGL(keys_kernel, dim3(blocks), dim3(kBlock), 0, s, d_poses_xyt, d_weights, n64,
                     1.0 / static_cast<double>(n64), c->bins, c->keys, c->q, c->ctrl);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(insert_kernel, dim3(blocks < kInsertBlocks ? blocks : kInsertBlocks), dim3(kBlock), 0, s, c->keys, c->q, n64, c->owner, c->slot_q,
                     c->slot_count, mask, c->bin_of, c->ctrl);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->ev[kPhaseBins], s));
  hipLaunchKernelGGL(count_kernel, dim3(tiles), dim3(kBlock), 0, s, c->owner, c->bin_of, n64, c->sums);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, s, c->sums, tiles, c->ctrl, &c->pinned.dev->bins);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(scatter_kernel, dim3(tiles), dim3(kBlock), 0, s, c->owner, c->bin_of, n64, c->sums,
                     c->bin_slot, c->bin_owner, c->rank_of_slot, c->lab, c->root_q, c->root_count);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(neighbours_kernel, dim3(blocks), dim3(kBlock), 0, s, c->keys, c->owner, c->rank_of_slot,
                     c->bin_owner, c->ctrl, mask, c->bins.n_theta, n64, c->nbr);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->ev[kPhaseLabels], s));
  const int rc = queue_rounds(c);
  if (rc != NDT2D_OK) return rc;
  c->launched = true;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_cluster_fetch(ndt2d_clusterer * c, ndt2d_cluster_header * header_out,
                        ndt2d_cluster_record * records_out, size_t capacity, size_t * n_records)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (n_records != nullptr) *n_records = 0;
  if (header_out == nullptr || n_records == nullptr || (records_out == nullptr && capacity > 0))
  {
    return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_fetch: null argument");
  }
  if (!c->launched && !c->fetched) return fail(c, NDT2D_ERR_STATE, "ndt2d_cluster_fetch: nothing launched");
  if (c->launched)
  {
    c->launched = false;
    std::memset(&c->result, 0, sizeof(Packed));
    if (c->n > 0)
    {
      NDT2D_OBJ_HIP(c, hipSetDevice(c->device));
      uint64_t rounds = 0;
      bool standing = false;
      uint64_t n_bins = 0;
      while (!standing)
      {
        NDT2D_OBJ_HIP(c, hipStreamSynchronize(c->stream));
        n_bins = __atomic_load_n(&c->pinned.host->bins, __ATOMIC_ACQUIRE);
        if (n_bins > c->n) return fail(c, NDT2D_ERR_INTERNAL, "ndt2d_cluster_fetch: more bins than particles");
        for (int r = 0; r < kRoundsPerRead && !standing; ++r)
        {
          ++rounds;
          standing = __atomic_load_n(&c->pinned.host->changed[r], __ATOMIC_ACQUIRE) == 0;
        }
        if (standing) break;
        // (plain propagation alone ends within B rounds)
        if (rounds > n_bins + 2) return fail(c, NDT2D_ERR_INTERNAL, "ndt2d_cluster_fetch: the labels did not stand still within B + 2 rounds");
        const int rc = queue_rounds(c);
        if (rc != NDT2D_OK) return rc;
      }
      if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->ev[kPhaseSelect], c->stream));
      const int rc = queue_rest(c);
      if (rc != NDT2D_OK) return rc;
      NDT2D_OBJ_HIP(c, hipStreamSynchronize(c->stream));
      if (c->pinned.host->packed.table_full != 0) return fail(c, NDT2D_ERR_INTERNAL, "ndt2d_cluster_fetch: the bin table ran out of slots");
      std::memcpy(&c->result, &c->pinned.host->packed, sizeof(Packed));
      c->result.header.rounds = rounds;
      c->timed = c->timing;
    }
    c->fetched = true;
  }
  *header_out = c->result.header;
  size_t live = 0;
  while (live < static_cast<size_t>(kMaxClusters) && c->result.records[live].label != fn::kLeftOut &&
         live < c->result.header.n_clusters)
  {
    ++live;
  }
  *n_records = live;
  if (capacity < live) return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_fetch: a capacity below the number of records");
  for (size_t k = 0; k < live; ++k) records_out[k] = c->result.records[k];
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_cluster_read_labels(ndt2d_clusterer * c, uint32_t * out, size_t n)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (!c->fetched) return fail(c, NDT2D_ERR_STATE, "ndt2d_cluster_read_labels: no fetched call");
  if (n != c->n) return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_read_labels: n is not the last call's");
  if (n == 0) return NDT2D_OK;
  if (out == nullptr) return fail(c, NDT2D_ERR_INVALID, "ndt2d_cluster_read_labels: null output");
  return ndt2d_copy_to_host(c->h, out, c->labels, n * sizeof(uint32_t));
  NDT2D_C_CATCH(c)
}

}  // extern "C"
