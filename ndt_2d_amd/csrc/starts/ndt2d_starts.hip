// Batched match from K start poses: ONE scan against the grid INSTALLED in the context, a full
// matchScan lattice around each of K starts, in one upload, one search launch, one reduction
// launch and one read-back (gfx950 / MI355X).
//
// Reference: a node that loads its map (src/ndt_mapper.cpp:106-116,155-186) refuses every scan
// until somebody posts `initialpose` (:315-320).  The remedy with this library -- matchScan
// (src/scan_matcher_ndt.cpp:76-150) from every graph node's pose under a few headings, keep the
// best response -- is K sequential searches, each one launch and one host round trip, each a
// lattice that fills a fraction of the chip.  The K searches are independent and read the same
// map, so here:
//
//   starts_search_kernel  grid (theta step, start), a lane per (dx, dy), as wide as the
//       translation lattice (wider lattices loop): the block rotates the beams once for
//       (theta_k + dth_i; cos / sin from the host libm, a table row per distinct start heading)
//       and its own (x_k, y_k) into LDS in pieces of kStageBeams, every lane adds points_inner =
//       outer + (dx, dy) (:121-125) through cell_index on the installed grid's geometry, the
//       occupancy bitmap, one 64-byte line of GridDesc::cells_global per scoring cell,
//       record_exponent / exp_score.  The walk is ../closure/ndt2d_walk_fn.h, shared with closure/.
//       K x n_theta blocks: 1,280 of seven waves for the plugin's defaults and K = 16, where one
//       sequential search is 80 x 7 tiles.
//   starts_reduce_kernel  one block per start: the n_theta records of its blocks ->
//       {best_score, best_index (+0.5: near tie), acc[10]} with merge_best, fixed order.
//
// Off the grid.  cell_index gives ncell for every point outside the grid, however far the start
// lies from the map; bit ncell of the bitmap is 0 and record ncell exists (the sentinel), so no
// lane indexes beyond either.  A start off the map scores 0.0 everywhere: no winner.
//
// The bits of a raw score are those of closure/: C in-order partial sums per lane over groups of
// four beams dealt round-robin, C from the beam count by the small-lattice search's default plan
// (../closure/ndt2d_sum_chunks.h), added ((p_0 + p_1) + p_2) + ...: the sequential search's bits wherever it
// runs the small-lattice search with that plan.  Terms are skipped by negligible_below(): bit-exact.
//
// Determinism.  As closure/: a lane's sums are its own, blocks reduce lanes over the DPP network
// and waves in wave order, the reducing block takes records r, r + 256, ... per thread.  Stream
// order is the only ordering between the two launches and __syncthreads the only barrier inside
// them; no polls, no atomics.  Two calls give the same bits, and so does any chunking of K.
//
// LDS of the search block: kStageBeams x {ox, oy} = 16 KB, reused for one record per wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "../closure/ndt2d_walk_fn.h"

namespace ndt2d
{

namespace
{

// One start of a launch.
struct StartRec
{
  double x, y;
  uint32_t trig_row;   // its heading's row of the cos / sin table
  uint32_t pad;
};
static_assert(sizeof(StartRec) == 3 * sizeof(double), "starts travel in a buffer of doubles");

struct StartsSearchArgs
{
  GridDesc grid;             // geometry, cells_global, occ_bits
  const StartRec * starts;
  const double * trig;       // [rows][2][n_th]: cos | sin of (heading + dth[i])
  const double * beams_xy;   // [n_beams][2] robot frame
  const double * dth, * dlin;
  uint32_t n_beams, n_th, n_lin;
  double * scores;           // optional: [start][n_th * n_lin * n_lin]
  double * partials;         // [start][n_th][kRecord]
};

// The installed grid as the lane's walk reads it: a cell is its own record.
struct InstalledMap
{
  const uint32_t * occ_bits;
  const double * cells_global;
  __device__ __forceinline__ bool find(uint32_t cell, uint32_t & rank) const
  {
    rank = cell;   // (<= ncell: bit ncell is 0)
    return ((occ_bits[cell >> 5] >> (cell & 31u)) & 1u) != 0u;
  }
  __device__ __forceinline__ const double2 * record(uint32_t rank) const
  {
    return reinterpret_cast<const double2 *>(cells_global + static_cast<size_t>(rank) * kCellStrideGlobal);
  }
};

template <int C, bool POW2>
__global__ void __launch_bounds__(kSearchMaxThreads) starts_search_kernel(const StartsSearchArgs a)
{
  __shared__ double2 rows[kStageBeams];
  const uint32_t ith = blockIdx.x, slot = blockIdx.y;
  const uint32_t tid = threadIdx.x, n_threads = blockDim.x;
  const StartRec s = a.starts[slot];
  const InstalledMap map{a.grid.occ_bits, a.grid.cells_global};
  const double * trig = a.trig + static_cast<size_t>(s.trig_row) * 2 * a.n_th;
  const double ct = trig[ith], st = trig[a.n_th + ith], dt = a.dth[ith];
  const uint32_t n_lin = a.n_lin, n_cand = n_lin * n_lin;

  double best_s = 0.0;       // `double best_score = 0;` (:83)
  double best_i = kNoIndex;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;

  for (uint32_t c0 = 0; c0 < n_cand; c0 += n_threads)
  {
    const uint32_t c = c0 + tid;
    const bool valid = c < n_cand;
    const uint32_t cc = valid ? c : n_cand - 1u;
    const uint32_t ix = cc / n_lin, iy = cc - ix * n_lin;
    const double dx = a.dlin[ix], dy = a.dlin[iy];
    const double sum = lane_walk<C, POW2>(a.grid, map, rows, a.beams_xy, a.n_beams, ct, st, s.x, s.y, dx, dy, valid);
    if (valid)
    {
      const double score = -sum;  // (:127)
      lane_take(score, static_cast<uint64_t>(ith) * n_cand + c, dx, dy, dt, best_s, best_i, acc);
      if (a.scores != nullptr) a.scores[(static_cast<uint64_t>(slot) * a.n_th + ith) * n_cand + c] = score;
    }
  }
  // the block's record (the rows are free behind block_record's first barrier)
  block_record<false>(best_s, best_i, acc, reinterpret_cast<double *>(rows),
                      a.partials + (static_cast<size_t>(slot) * a.n_th + ith) * kRecord);
}

// partials[start][n_th][kRecord] -> out[start][kRecord]
__global__ void __launch_bounds__(kReduceThreads) starts_reduce_kernel(const double * partials, uint32_t n_th,
                                                                        double * out)
{
  __shared__ double scratch[(kReduceThreads / 64) * kRecord];
  const uint32_t slot = blockIdx.x;
  reduce_slot_records(partials + static_cast<size_t>(slot) * n_th * kRecord, n_th, scratch,
                      out + static_cast<size_t>(slot) * kRecord);
}

template <bool POW2>
void launch_search_c(uint32_t chunks, dim3 grid, dim3 block, hipStream_t stream, const StartsSearchArgs & a)
{
  switch (chunks)
  {
    case 1: hipLaunchKernelGGL((starts_search_kernel<1, POW2>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((starts_search_kernel<2, POW2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((starts_search_kernel<3, POW2>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((starts_search_kernel<4, POW2>), grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL((starts_search_kernel<5, POW2>), grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL((starts_search_kernel<6, POW2>), grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL((starts_search_kernel<7, POW2>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((starts_search_kernel<8, POW2>), grid, block, 0, stream, a); break;
  }
}

}  // namespace

}  // namespace ndt2d

// ---- the object and the C entry points ----

struct ndt2d_starts
{
  ndt2d_handle h = nullptr;
  int device = 0;
  size_t max_starts = 0;
  std::string err;
  // one upload per chunk: [dth | dlin | beams | starts | cos / sin rows] (doubles), pinned and on the device
  double * h_stage = nullptr, * d_stage = nullptr;
  size_t stage_cap = 0;
  void * d_partials = nullptr;
  size_t partials_cap = 0;   // bytes
  // what comes back: [start][12] records | [start][lattice] scores (doubles), on the device and pinned
  double * d_out = nullptr, * h_out = nullptr;
  size_t out_cap = 0;
  std::vector<double> trig;                        // the chunk's cos / sin rows
  std::unordered_map<uint64_t, uint32_t> row_of;   // heading (bits) -> row
  bool timing = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // before the search, behind it, behind the reduction
  bool timed = false;
};

namespace
{

using ndt2d::GridDesc;
using ndt2d::StartRec;
constexpr size_t kRec = NDT2D_MATCH_RECORD_DOUBLES;
// all_scores wanted: starts of one launch, so that the scores on their way back stay within this
constexpr size_t kScoreDoublesPerLaunch = size_t(8) << 20;

void guard_note(ndt2d_starts * s, const char * what) noexcept
{
  if (s == nullptr) return;
  try
  {
    s->err = what;
  }
  catch (...)
  {
  }
}
void guard_note(std::nullptr_t, const char *) noexcept {}

int sfail(ndt2d_starts * s, int code, const std::string & msg)
{
  if (s != nullptr) s->err = msg;
  return code;
}

int sfail_hip(ndt2d_starts * s, hipError_t e, const char * what)
{
  (void)hipGetLastError();  // clear sticky state
  return sfail(s, NDT2D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define NDT2D_STARTS_HIP(s, call)                           \
  do                                                        \
  {                                                         \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return sfail_hip(s, e__, #call); \
  } while (0)

// A pinned / device pair of at least `doubles` (contents are not kept).
hipError_t grow_pair(double ** host, double ** dev, size_t * cap, size_t doubles)
{
  if (doubles <= *cap) return hipSuccess;
  *cap = 0;
  if (*host != nullptr) (void)hipHostFree(*host);
  if (*dev != nullptr) (void)hipFree(*dev);
  *host = nullptr;
  *dev = nullptr;
  const size_t want = doubles + doubles / 4 + 512;
  hipError_t e = hipHostMalloc(reinterpret_cast<void **>(host), want * sizeof(double), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(dev), want * sizeof(double));
  if (e == hipSuccess) *cap = want;
  return e;
}

void free_starts(ndt2d_starts * s)
{
  (void)hipSetDevice(s->device);
  if (s->h_stage != nullptr) (void)hipHostFree(s->h_stage);
  if (s->d_stage != nullptr) (void)hipFree(s->d_stage);
  if (s->d_partials != nullptr) (void)hipFree(s->d_partials);
  if (s->d_out != nullptr) (void)hipFree(s->d_out);
  if (s->h_out != nullptr) (void)hipHostFree(s->h_out);
  for (hipEvent_t ev : s->ev)
  {
    if (ev != nullptr) (void)hipEventDestroy(ev);
  }
  delete s;
}

struct SearchTables
{
  const double * beams_xy;
  size_t n_beams;
  const double * dth;
  size_t n_th;
  const double * dlin;
  size_t n_lin;
};

// Starts [k0, k1) of a call whose arguments have been checked.  records_out / all_scores: the call's, whole.
int match_chunk(ndt2d_starts * s, const GridDesc & grid, size_t k0, size_t k1, const double * starts_xyt,
                const SearchTables & t, double * records_out, double * all_scores)
{
  const size_t n_slots = k1 - k0;
  const size_t n_lattice = t.n_th * t.n_lin * t.n_lin;
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));

  // cos / sin of (heading + dth[i]) from the host libm (:106-107), a row per distinct heading
  s->row_of.clear();
  s->trig.clear();
  std::vector<uint32_t> rows(n_slots);
  for (size_t k = k0; k < k1; ++k)
  {
    const double theta = starts_xyt[3 * k + 2];
    uint64_t bits;
    std::memcpy(&bits, &theta, sizeof(bits));
    auto it = s->row_of.find(bits);
    if (it == s->row_of.end())
    {
      const uint32_t row = static_cast<uint32_t>(s->trig.size() / (2 * t.n_th));
      it = s->row_of.emplace(bits, row).first;
      s->trig.resize(s->trig.size() + 2 * t.n_th);
      double * c = s->trig.data() + static_cast<size_t>(row) * 2 * t.n_th;
      for (size_t i = 0; i < t.n_th; ++i) ndt2d_cos_sin(theta + t.dth[i], c + i, c + t.n_th + i);
    }
    rows[k - k0] = it->second;
  }

  // [dth | dlin | beams | starts | cos / sin rows]
  const size_t off_beams = (t.n_th + t.n_lin + 1) & ~size_t(1);   // (beams: 16-byte loads)
  const size_t off_starts = off_beams + 2 * t.n_beams;
  const size_t off_trig = off_starts + n_slots * (sizeof(StartRec) / sizeof(double));
  const size_t n_stage = off_trig + s->trig.size();
  NDT2D_STARTS_HIP(s, grow_pair(&s->h_stage, &s->d_stage, &s->stage_cap, n_stage));
  const size_t partial_bytes = n_slots * t.n_th * kRec * sizeof(double);
  if (partial_bytes > s->partials_cap)
  {
    if (s->d_partials != nullptr) (void)hipFree(s->d_partials);
    s->d_partials = nullptr;
    s->partials_cap = 0;
    const size_t want = partial_bytes + partial_bytes / 4;
    NDT2D_STARTS_HIP(s, hipMalloc(&s->d_partials, want));
    s->partials_cap = want;
  }
  const size_t n_out = n_slots * (kRec + (all_scores != nullptr ? n_lattice : 0));
  NDT2D_STARTS_HIP(s, grow_pair(&s->h_out, &s->d_out, &s->out_cap, n_out));

  double * st = s->h_stage;
  std::memcpy(st, t.dth, t.n_th * sizeof(double));
  std::memcpy(st + t.n_th, t.dlin, t.n_lin * sizeof(double));
  std::memcpy(st + off_beams, t.beams_xy, 2 * t.n_beams * sizeof(double));
  StartRec * recs = reinterpret_cast<StartRec *>(st + off_starts);
  for (size_t k = k0; k < k1; ++k)
  {
    recs[k - k0] = StartRec{starts_xyt[3 * k], starts_xyt[3 * k + 1], rows[k - k0], 0u};
  }
  std::memcpy(st + off_trig, s->trig.data(), s->trig.size() * sizeof(double));

  // the one upload of the chunk
  NDT2D_STARTS_HIP(s, hipMemcpyAsync(s->d_stage, st, n_stage * sizeof(double), hipMemcpyHostToDevice, stream));
  s->timed = false;
  if (s->timing) NDT2D_STARTS_HIP(s, hipEventRecord(s->ev[0], stream));

  ndt2d::StartsSearchArgs a{};
  a.grid = grid;
  a.starts = reinterpret_cast<const StartRec *>(s->d_stage + off_starts);
  a.trig = s->d_stage + off_trig;
  a.beams_xy = s->d_stage + off_beams;
  a.dth = s->d_stage;
  a.dlin = s->d_stage + t.n_th;
  a.n_beams = static_cast<uint32_t>(t.n_beams);
  a.n_th = static_cast<uint32_t>(t.n_th);
  a.n_lin = static_cast<uint32_t>(t.n_lin);
  a.scores = all_scores != nullptr ? s->d_out + n_slots * kRec : nullptr;
  a.partials = static_cast<double *>(s->d_partials);
  const size_t n_cand = t.n_lin * t.n_lin;
  const uint32_t threads = static_cast<uint32_t>(std::min<size_t>(ndt2d::kSearchMaxThreads, (n_cand + 63) & ~size_t(63)));
  const dim3 grid_dim(static_cast<uint32_t>(t.n_th), static_cast<uint32_t>(n_slots));
  const uint32_t chunks = ndt2d::sum_chunks(a.n_beams);
  if (grid.pow2) ndt2d::launch_search_c<true>(chunks, grid_dim, dim3(threads), stream, a);
  else ndt2d::launch_search_c<false>(chunks, grid_dim, dim3(threads), stream, a);
  NDT2D_STARTS_HIP(s, hipGetLastError());
  if (s->timing) NDT2D_STARTS_HIP(s, hipEventRecord(s->ev[1], stream));

  hipLaunchKernelGGL(ndt2d::starts_reduce_kernel, dim3(static_cast<uint32_t>(n_slots)), dim3(ndt2d::kReduceThreads), 0,
                     stream, a.partials, a.n_th, s->d_out);
  NDT2D_STARTS_HIP(s, hipGetLastError());
  if (s->timing) NDT2D_STARTS_HIP(s, hipEventRecord(s->ev[2], stream));
  // the one read-back of the chunk
  NDT2D_STARTS_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, stream));
  NDT2D_STARTS_HIP(s, hipStreamSynchronize(stream));
  s->timed = s->timing;
  std::memcpy(records_out + k0 * kRec, s->h_out, n_slots * kRec * sizeof(double));
  if (all_scores != nullptr)
  {
    std::memcpy(all_scores + k0 * n_lattice, s->h_out + n_slots * kRec, n_slots * n_lattice * sizeof(double));
  }
  return NDT2D_OK;
}

}  // namespace

extern "C" {

int ndt2d_starts_create(ndt2d_handle h, size_t max_starts, ndt2d_starts ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || max_starts == 0 || max_starts > 4096) return NDT2D_ERR_INVALID;
  ndt2d_starts * s = new ndt2d_starts();
  s->h = h;
  s->device = ndt2d_device_id(h);
  s->max_starts = max_starts;
  *out = s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_starts_destroy(ndt2d_starts * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(s->h)));
  free_starts(s);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_starts_last_error(ndt2d_starts * s)
{
  return s != nullptr ? s->err.c_str() : "null starts";
}

int ndt2d_starts_set_timing(ndt2d_starts * s, int enabled)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (enabled != 0 && s->ev[0] == nullptr)
  {
    NDT2D_STARTS_HIP(s, hipSetDevice(s->device));
    for (hipEvent_t & ev : s->ev) NDT2D_STARTS_HIP(s, hipEventCreate(&ev));
  }
  s->timing = enabled != 0;
  s->timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_starts_last_ms(ndt2d_starts * s, float * search_ms, float * reduce_ms)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (!s->timed) return sfail(s, NDT2D_ERR_STATE, "ndt2d_starts_last_ms: no timed match (ndt2d_starts_set_timing)");
  float a = 0.0f, b = 0.0f;
  NDT2D_STARTS_HIP(s, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  NDT2D_STARTS_HIP(s, hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
  if (search_ms != nullptr) *search_ms = a;
  if (reduce_ms != nullptr) *reduce_ms = b;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_starts_match(ndt2d_starts * s, const double * starts_xyt, size_t n_starts, const double * beams_xy,
                       size_t n_beams, const double * dth, size_t n_th, const double * dlin, size_t n_lin,
                       double * records_out, double * all_scores)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_starts == 0) return NDT2D_OK;
  if (starts_xyt == nullptr || records_out == nullptr || beams_xy == nullptr || dth == nullptr || dlin == nullptr)
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: null argument");
  }
  // what ndt2d_set_beams / ndt2d_set_search refuse
  if (n_beams == 0 || n_beams > (1u << 20)) return sfail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: bad argument (n_beams)");
  if (n_th == 0 || n_lin == 0 || n_th > (1u << 24) || n_lin > 46340)
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: bad argument (lattice)");
  }
  if (n_starts >= (1u << 24)) return sfail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: bad argument (n_starts)");
  // every start is checked before anything is launched
  for (size_t k = 0; k < n_starts; ++k)
  {
    if (!std::isfinite(starts_xyt[3 * k]) || !std::isfinite(starts_xyt[3 * k + 1]) || !std::isfinite(starts_xyt[3 * k + 2]))
    {
      return sfail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: start " + std::to_string(k) + ": the pose is not finite");
    }
  }
  // the grid installed NOW; a list install's deferred map bytes are not read here and stay deferred
  ndt2d_grid_view v;
  const int vrc = ndt2d_grid_view_get(s->h, &v);
  if (vrc != NDT2D_OK) return sfail(s, vrc, vrc == NDT2D_ERR_NO_GRID ? "ndt2d_starts_match: no grid" : "ndt2d_starts_match: no grid view");
  GridDesc grid{};
  grid.cells_global = v.cells_global;
  grid.occ_bits = v.occ_bits;
  grid.size_x = v.size_x;
  grid.size_y = v.size_y;
  grid.ncell = v.ncell;
  grid.pow2 = v.pow2;
  grid.cell_size = v.cell_size;
  grid.inv_cell_size = v.inv_cell_size;
  grid.origin_x = v.origin_x;
  grid.origin_y = v.origin_y;
  if (grid.cells_global == nullptr || grid.occ_bits == nullptr)
  {
    return sfail(s, NDT2D_ERR_STATE, "ndt2d_starts_match: the installed grid has no records");
  }
  NDT2D_STARTS_HIP(s, hipSetDevice(s->device));
  const SearchTables t{beams_xy, n_beams, dth, n_th, dlin, n_lin};
  // more starts than slots: in chunks
  size_t per_launch = s->max_starts;
  if (all_scores != nullptr)
  {
    const size_t n_lattice = n_th * n_lin * n_lin;
    per_launch = std::min(per_launch, std::max<size_t>(1, kScoreDoublesPerLaunch / n_lattice));
  }
  for (size_t k0 = 0; k0 < n_starts; k0 += per_launch)
  {
    const size_t k1 = std::min(n_starts, k0 + per_launch);
    const int rc = match_chunk(s, grid, k0, k1, starts_xyt, t, records_out, all_scores);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
