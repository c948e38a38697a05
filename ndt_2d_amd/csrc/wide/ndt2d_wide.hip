// Wide search: the winner of an exhaustive (x, y, theta) lattice -- its score bits, its index and
// its near-tie mark -- without scoring most of the lattice (gfx950 / MI355X).
//
// Reference: matchScan (src/scan_matcher_ndt.cpp:76-150) scores every candidate of the lattice and
// keeps the best under a strict `<` (:128).  Relocalisation and loop closure after drift want
// windows of metres and radians: hundreds of millions of candidates, nearly all of them far from
// plausible.  A RIGOROUS upper bound on the best likelihood sum inside a small tile of the
// translation lattice costs one table look-up per beam; a tile whose bound lies below a sum
// already achieved holds no winner and nothing within the near-tie tolerance of one, and is never
// scored.  What is scored is scored by lane_walk (../batch/ndt2d_walk_fn.h), so a candidate's raw
// sum has the bits ndt2d_starts_match gives it.
//
//   wide_image_kernel    a thread per pixel of the bound image (ndt2d_wide_fn.h: the exact maximum
//                        of every touched cell's exponent over the pixel's box, exp, inflated).
//   wide_bounds_kernel   a wave per tile job (theta step, tile), lanes over beams: the beam rotated
//                        as lane_walk rotates it, moved to the tile's lower corner, looked up; lane
//                        sums in beam order, lanes over the fixed xor tree.  FP64, no atomics.
//   rocprim radix sort   (bound bits, job) descending, stable: ties stay in ascending job order.
//   wide_exact_kernel<C, POW2>   a block per tile job of a chunk of the sorted list, a lane per
//                        candidate of the tile: lane_walk, the reference's `score < 0` rule, the flat
//                        index in the FULL lattice, the block's (score, index) by merge_best.
//   wide_reduce_kernel   the chunk's records into the running record; leaves it with the bound at
//                        the next chunk's head for the one small read-back of the round.
//
// The host walks the sorted jobs in chunks that double up to max_tiles and stops when the next
// bound is strictly below best_sum (1 - 2^-35): every candidate within merge_best's 2^-36 of the
// winner has then met it.  The covariance sums acc[10] need every candidate and are not made.
//
// Determinism.  A lane's sums are its own; blocks reduce lanes over the DPP network and waves in
// wave order; the reducing block takes records r, r + 256, ... per thread.  Stream order is the only
// ordering between launches; no polls, no atomics.  Which tiles are scored depends on the bounds
// and the scores alone, so two calls score the same tiles.
//
// Off the grid.  The exact kernel is lane_walk's: cell_index gives ncell for a point outside, bit
// ncell is 0.  The image kernel indexes cells inside [0, size) only (cell_range clamps), the bounds
// kernel pixels inside [0, nx) x [0, ny) only (pixel_of refuses the rest, NaN included), the exact
// kernel jobs below n_jobs from a sorted list of n_jobs entries.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "batch/ndt2d_installed_map.h"
#include "batch/ndt2d_walk_fn.h"
#include "wide/ndt2d_wide_fn.h"

struct ndt2d_wide : ndt2d::BatchHost
{
  size_t max_tiles = 0;
  uint32_t tile_steps = NDT2D_WIDE_DEFAULT_TILE_STEPS;
  uint32_t pixels_per_tile = NDT2D_WIDE_DEFAULT_PIXELS_PER_TILE;
  // the image of the last call that made one
  ndt2d::wide::Image image{};
  bool have_image = false;
  double * d_image = nullptr;
  size_t image_cap = 0;                       // bytes
  // per tile job: bound bits and job, unsorted | sorted; the evaluated bytes; the sort's scratch
  void * d_jobs = nullptr;
  size_t jobs_cap = 0;
  void * d_sort_temp = nullptr;
  size_t sort_temp_cap = 0;
  std::vector<double> trig;
  hipEvent_t stage_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool stage_timed = false;
};

namespace ndt2d
{

namespace
{

constexpr uint32_t kImageThreads = 256;
constexpr uint32_t kBoundsThreads = 256;    // four jobs of a wave each
constexpr size_t kFirstChunk = 64;          // tile jobs of the first exact round

struct WideLattice
{
  const double * dth, * dlin;    // device
  const double * cos_th, * sin_th;
  const double * beams_xy;
  uint32_t n_th, n_lin, n_beams;
  uint32_t tile_steps, n_tiles;  // tiles along an axis
  double pose_x, pose_y;
};

__global__ void __launch_bounds__(kImageThreads) wide_image_kernel(const wide::GridRef g, const wide::Image im, double * out)
{
  const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kImageThreads + threadIdx.x;
  if (p >= static_cast<uint64_t>(im.nx) * im.ny) return;
  const uint32_t j = static_cast<uint32_t>(p / im.nx), i = static_cast<uint32_t>(p - static_cast<uint64_t>(j) * im.nx);
  out[p] = wide::pixel_value(g, im, i, j);
}

// keys[job] = the bits of the job's bound (a non-negative double: its bits sort as it does),
// vals[job] = job.
__global__ void __launch_bounds__(kBoundsThreads) wide_bounds_kernel(const WideLattice a, const wide::Image im,
                                                                      const double * __restrict__ image, uint32_t n_jobs,
                                                                      uint64_t * keys, uint32_t * vals)
{
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t job = blockIdx.x * (kBoundsThreads / kWave) + (threadIdx.x >> 6);
  if (job >= n_jobs) return;   // (whole waves: no barrier follows)
  const uint32_t per_th = a.n_tiles * a.n_tiles;
  const uint32_t ith = job / per_th, t = job - ith * per_th;
  const uint32_t tx = t / a.n_tiles, ty = t - tx * a.n_tiles;
  const double ct = a.cos_th[ith], st = a.sin_th[ith];
  const double dx = a.dlin[tx * a.tile_steps], dy = a.dlin[ty * a.tile_steps];
  double sum = 0.0;
  for (uint32_t b = lane; b < a.n_beams; b += kWave)
  {
    const double2 q = reinterpret_cast<const double2 *>(a.beams_xy)[b];
    // points_outer as lane_walk has it, then the tile's lower corner
    const double ox = q.x * ct - q.y * st + a.pose_x;
    const double oy = q.x * st + q.y * ct + a.pose_y;
    uint32_t i, j;
    if (wide::pixel_of(im, ox + dx, oy + dy, i, j)) sum += image[static_cast<size_t>(j) * im.nx + i];
  }
  sum = wave_sum(sum);
  if (lane == 0)
  {
    keys[job] = static_cast<uint64_t>(__double_as_longlong(wide::tile_bound(sum, a.n_beams)));
    vals[job] = job;
  }
}

// A block per tile job sorted[first + blockIdx.x], a lane per candidate of the tile.
template <int C, bool POW2>
__global__ void __launch_bounds__(kSearchMaxThreads) wide_exact_kernel(const GridDesc g, const WideLattice a,
                                                                       const uint32_t * sorted_jobs, uint32_t first,
                                                                       double * partials, uint8_t * evaluated)
{
  __shared__ double2 rows[kStageBeams];
  const uint32_t tid = threadIdx.x;
  const uint32_t job = sorted_jobs[first + blockIdx.x];
  const uint32_t per_th = a.n_tiles * a.n_tiles;
  const uint32_t ith = job / per_th, t = job - ith * per_th;
  const uint32_t tx = t / a.n_tiles, ty = t - tx * a.n_tiles;
  const uint32_t lx = tid / a.tile_steps, ly = tid - lx * a.tile_steps;
  const uint32_t ix = tx * a.tile_steps + lx, iy = ty * a.tile_steps + ly;
  const bool valid = (lx < a.tile_steps) & (ix < a.n_lin) & (iy < a.n_lin);
  const double dx = a.dlin[min(ix, a.n_lin - 1u)], dy = a.dlin[min(iy, a.n_lin - 1u)];
  const InstalledMap map{g.occ_bits, g.cells_global};
  const double sum = lane_walk<C, POW2>(g, map, rows, a.beams_xy, a.n_beams, a.cos_th[ith], a.sin_th[ith], a.pose_x,
                                        a.pose_y, dx, dy, valid);
  double best_s = 0.0, best_i = kNoIndex;   // `double best_score = 0;` (:83)
  const double score = -sum;                // (:127)
  if (valid & (score < 0.0))
  {
    best_s = score;
    best_i = static_cast<double>((static_cast<uint64_t>(ith) * a.n_lin + ix) * a.n_lin + iy);
  }
  wave_best_to_last_lane(best_s, best_i);
  double * scratch = reinterpret_cast<double *>(rows);
  const uint32_t lane = tid & (kWave - 1), wave = tid >> 6, n_waves = blockDim.x >> 6;
  __syncthreads();   // the rows have been read
  if (lane == kWave - 1)
  {
    scratch[2 * wave] = best_s;
    scratch[2 * wave + 1] = best_i;
  }
  __syncthreads();
  if (tid == 0)
  {
    double s0 = scratch[0], i0 = scratch[1];
    for (uint32_t w = 1; w < n_waves; ++w) merge_best(scratch[2 * w], scratch[2 * w + 1], s0, i0);
    partials[2 * static_cast<size_t>(blockIdx.x)] = s0;
    partials[2 * static_cast<size_t>(blockIdx.x) + 1] = i0;
    evaluated[job] = 1;
  }
}

// record {score, index (kNoIndex: none)}: the running record merged with the chunk's n records;
// out = {score, index, the bound at sorted position `next` (or -1: the list is at its end)}.
__global__ void __launch_bounds__(kReduceThreads) wide_reduce_kernel(const double * partials, uint32_t n, double * record,
                                                                      const uint64_t * sorted_keys, uint32_t next,
                                                                      uint32_t n_jobs, double * out)
{
  __shared__ double scratch[2 * (kReduceThreads / kWave)];
  const uint32_t tid = threadIdx.x;
  double bs = 0.0, bi = kNoIndex;
  if (tid == 0)
  {
    bs = record[0];
    bi = record[1];
  }
  for (uint32_t r = tid; r < n; r += kReduceThreads) merge_best(partials[2 * r], partials[2 * r + 1], bs, bi);
  wave_best_to_last_lane(bs, bi);
  const uint32_t lane = tid & (kWave - 1), wave = tid >> 6;
  if (lane == kWave - 1)
  {
    scratch[2 * wave] = bs;
    scratch[2 * wave + 1] = bi;
  }
  __syncthreads();
  if (tid == 0)
  {
    double s0 = scratch[0], i0 = scratch[1];
    for (uint32_t w = 1; w < kReduceThreads / kWave; ++w) merge_best(scratch[2 * w], scratch[2 * w + 1], s0, i0);
    record[0] = s0;
    record[1] = i0;
    out[0] = s0;
    out[1] = i0;
    out[2] = next < n_jobs ? __longlong_as_double(static_cast<long long>(sorted_keys[next])) : -1.0;
  }
}

template <int C>
void launch_exact_c(bool pow2, uint32_t blocks, uint32_t threads, hipStream_t stream, const GridDesc & g, const WideLattice & a,
                    const uint32_t * sorted_jobs, uint32_t first, double * partials, uint8_t * evaluated)
{
  if (pow2) hipLaunchKernelGGL((wide_exact_kernel<C, true>), dim3(blocks), dim3(threads), 0, stream, g, a, sorted_jobs, first, partials, evaluated);
  else hipLaunchKernelGGL((wide_exact_kernel<C, false>), dim3(blocks), dim3(threads), 0, stream, g, a, sorted_jobs, first, partials, evaluated);
}

void launch_exact(uint32_t chunks, bool pow2, uint32_t blocks, uint32_t threads, hipStream_t stream, const GridDesc & g,
                  const WideLattice & a, const uint32_t * sorted_jobs, uint32_t first, double * partials, uint8_t * evaluated)
{
  switch (chunks)
  {
    case 1: launch_exact_c<1>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
    case 2: launch_exact_c<2>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
    case 3: launch_exact_c<3>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
    case 4: launch_exact_c<4>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
    case 5: launch_exact_c<5>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
    case 6: launch_exact_c<6>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
    case 7: launch_exact_c<7>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
    default: launch_exact_c<8>(pow2, blocks, threads, stream, g, a, sorted_jobs, first, partials, evaluated); break;
  }
}

size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// Where the per-job arrays lie in d_jobs (bytes).
struct JobsLayout
{
  size_t keys_in, keys_out, vals_in, vals_out, evaluated, total;
};
JobsLayout jobs_layout(size_t n_jobs)
{
  JobsLayout at;
  at.keys_in = 0;
  at.keys_out = at.keys_in + round_up(n_jobs * 8, 256);
  at.vals_in = at.keys_out + round_up(n_jobs * 8, 256);
  at.vals_out = at.vals_in + round_up(n_jobs * 4, 256);
  at.evaluated = at.vals_out + round_up(n_jobs * 4, 256);
  at.total = at.evaluated + round_up(n_jobs, 256);
  return at;
}

int wide_match(ndt2d_wide * w, const double * pose_xyt, const double * beams_xy, size_t n_beams, const double * dth,
               size_t n_th, const double * dlin, size_t n_lin, int reuse_image, double * record_out, uint64_t * stats_out,
               double * bounds_out, uint8_t * evaluated_out)
{
  const char * who = "ndt2d_wide_match";
  int rc = NDT2D_OK;
  const GridDesc grid = installed_grid(w->h, &rc);
  if (rc != NDT2D_OK)
  {
    return batch_fail(w, rc, std::string(who) + (rc == NDT2D_ERR_NO_GRID ? ": no grid"
                                                 : rc == NDT2D_ERR_STATE ? ": the installed grid has no records"
                                                                         : ": no grid view"));
  }
  // the tiles of the call and the widest window among them
  const size_t T = w->tile_steps;
  const size_t n_tiles = (n_lin + T - 1) / T;
  double window = 0.0;
  for (size_t i0 = 0; i0 < n_lin; i0 += T)
  {
    const size_t last = std::min(n_lin, i0 + T) - 1;
    window = std::max(window, dlin[last] - dlin[i0]);
  }
  const size_t n_jobs = n_th * n_tiles * n_tiles;
  if (n_jobs >= (size_t(1) << 31))
  {
    return batch_fail(w, NDT2D_ERR_INVALID, std::string(who) + ": more than 2^31 - 1 tile jobs (ndt2d_wide_set_tile: more tile steps, or a smaller lattice)");
  }
  wide::Image im{};
  im.window = window;
  im.pitch = wide::pitch_of(window, grid.cell_size, w->pixels_per_tile);
  im.inv_pitch = 1.0 / im.pitch;
  im.origin_x = grid.origin_x - (window + im.pitch);
  im.origin_y = grid.origin_y - (window + im.pitch);
  if (!std::isfinite(im.inv_pitch) || !(im.pitch > 1.0e3 * wide::kGuard))
  {
    return batch_fail(w, NDT2D_ERR_INVALID, std::string(who) + ": the pixel pitch is not finite or below a micrometre");
  }
  if (wide::box_cells_along(window, im.pitch, grid.cell_size) > static_cast<double>(wide::kMaxBoxCells))
  {
    return batch_fail(w, NDT2D_ERR_INVALID, std::string(who) + ": a pixel's box spans more than 8 x 8 cells: the tile is too coarse to prune anything "
                                            "(ndt2d_wide_set_tile: fewer tile steps, or ndt2d_starts_match for this lattice)");
  }
  const double nx = wide::pixels_along(grid.size_x, grid.cell_size, window, im.pitch);
  const double ny = wide::pixels_along(grid.size_y, grid.cell_size, window, im.pitch);
  if (!(nx * ny <= static_cast<double>(wide::kMaxPixels)))
  {
    return batch_fail(w, NDT2D_ERR_INVALID, std::string(who) + ": the bound image would have more than 2^26 pixels "
                                            "(ndt2d_wide_set_tile: more tile steps or fewer pixels per tile)");
  }
  im.nx = static_cast<uint32_t>(nx);
  im.ny = static_cast<uint32_t>(ny);
  const size_t n_pixels = static_cast<size_t>(im.nx) * im.ny;

  NDT2D_BATCH_HIP(w, hipSetDevice(w->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(w->h));

  // the one upload: [dth | dlin | beams | cos | sin]; what comes back per round: 3 doubles
  const size_t off_dth = 0, off_dlin = off_dth + n_th, off_beams = (off_dlin + n_lin + 1) & ~size_t(1);
  const size_t off_cos = off_beams + 2 * n_beams, off_sin = off_cos + n_th, stage_total = off_sin + n_th;
  const size_t max_chunk = std::min(w->max_tiles, n_jobs);
  NDT2D_BATCH_HIP(w, grow_pair(&w->h_stage, &w->d_stage, &w->stage_cap, stage_total));
  NDT2D_BATCH_HIP(w, grow_pair(&w->h_out, &w->d_out, &w->out_cap, 8));
  NDT2D_BATCH_HIP(w, grow_device(&w->d_partials, &w->partials_cap, 2 * max_chunk * sizeof(double)));
  const JobsLayout at = jobs_layout(n_jobs);
  NDT2D_BATCH_HIP(w, grow_device(&w->d_jobs, &w->jobs_cap, at.total));
  const bool same_image = w->have_image && w->image.nx == im.nx && w->image.ny == im.ny && w->image.pitch == im.pitch &&
                          w->image.window == im.window && w->image.origin_x == im.origin_x && w->image.origin_y == im.origin_y;
  const bool make_image = !(reuse_image != 0 && same_image);
  if (make_image)
  {
    w->have_image = false;
    NDT2D_BATCH_HIP(w, grow_device(reinterpret_cast<void **>(&w->d_image), &w->image_cap, n_pixels * sizeof(double)));
  }
  char * jobs = static_cast<char *>(w->d_jobs);
  uint64_t * keys_in = reinterpret_cast<uint64_t *>(jobs + at.keys_in), * keys_out = reinterpret_cast<uint64_t *>(jobs + at.keys_out);
  uint32_t * vals_in = reinterpret_cast<uint32_t *>(jobs + at.vals_in), * vals_out = reinterpret_cast<uint32_t *>(jobs + at.vals_out);
  uint8_t * evaluated = reinterpret_cast<uint8_t *>(jobs + at.evaluated);
  size_t sort_bytes = 0;
  NDT2D_BATCH_HIP(w, rocprim::radix_sort_pairs_desc(nullptr, sort_bytes, keys_in, keys_out, vals_in, vals_out, n_jobs, 0u, 64u, stream));
  NDT2D_BATCH_HIP(w, grow_device(&w->d_sort_temp, &w->sort_temp_cap, std::max<size_t>(sort_bytes, 256)));

  double * st = w->h_stage;
  std::memcpy(st + off_dth, dth, n_th * sizeof(double));
  std::memcpy(st + off_dlin, dlin, n_lin * sizeof(double));
  if (off_beams > off_dlin + n_lin) st[off_beams - 1] = 0.0;   // (the beams start on 16 bytes)
  std::memcpy(st + off_beams, beams_xy, 2 * n_beams * sizeof(double));
  // cos / sin of (heading + dth[i]) from the host libm (src/scan_matcher_ndt.cpp:106-107)
  for (size_t i = 0; i < n_th; ++i) ndt2d_cos_sin(pose_xyt[2] + dth[i], st + off_cos + i, st + off_sin + i);
  NDT2D_BATCH_HIP(w, hipMemcpyAsync(w->d_stage, st, stage_total * sizeof(double), hipMemcpyHostToDevice, stream));
  NDT2D_BATCH_HIP(w, hipMemsetAsync(evaluated, 0, n_jobs, stream));
  w->h_out[0] = 0.0;
  w->h_out[1] = kNoIndex;
  NDT2D_BATCH_HIP(w, hipMemcpyAsync(w->d_out + 4, w->h_out, 2 * sizeof(double), hipMemcpyHostToDevice, stream));   // the running record

  WideLattice a{};
  a.dth = w->d_stage + off_dth;
  a.dlin = w->d_stage + off_dlin;
  a.beams_xy = w->d_stage + off_beams;
  a.cos_th = w->d_stage + off_cos;
  a.sin_th = w->d_stage + off_sin;
  a.n_th = static_cast<uint32_t>(n_th);
  a.n_lin = static_cast<uint32_t>(n_lin);
  a.n_beams = static_cast<uint32_t>(n_beams);
  a.tile_steps = static_cast<uint32_t>(T);
  a.n_tiles = static_cast<uint32_t>(n_tiles);
  a.pose_x = pose_xyt[0];
  a.pose_y = pose_xyt[1];

  w->stage_timed = false;
  const bool timing = w->timing;
  if (timing) NDT2D_BATCH_HIP(w, hipEventRecord(w->stage_ev[0], stream));
  if (make_image)
  {
    const wide::GridRef gref{grid.cells_global, grid.occ_bits, static_cast<uint32_t>(kCellStrideGlobal), grid.size_x, grid.size_y,
                             grid.cell_size, grid.origin_x, grid.origin_y};
    hipLaunchKernelGGL(wide_image_kernel, dim3(static_cast<uint32_t>((n_pixels + kImageThreads - 1) / kImageThreads)),
                       dim3(kImageThreads), 0, stream, gref, im, w->d_image);
    NDT2D_BATCH_HIP(w, hipGetLastError());
    w->image = im;
    w->have_image = true;
  }
  if (timing) NDT2D_BATCH_HIP(w, hipEventRecord(w->stage_ev[1], stream));
  const uint32_t jobs_per_block = kBoundsThreads / kWave;
  hipLaunchKernelGGL(wide_bounds_kernel, dim3(static_cast<uint32_t>((n_jobs + jobs_per_block - 1) / jobs_per_block)),
                     dim3(kBoundsThreads), 0, stream, a, im, static_cast<const double *>(w->d_image),
                     static_cast<uint32_t>(n_jobs), keys_in, vals_in);
  NDT2D_BATCH_HIP(w, hipGetLastError());
  if (timing) NDT2D_BATCH_HIP(w, hipEventRecord(w->stage_ev[2], stream));
  size_t temp = w->sort_temp_cap;
  NDT2D_BATCH_HIP(w, rocprim::radix_sort_pairs_desc(w->d_sort_temp, temp, keys_in, keys_out, vals_in, vals_out, n_jobs, 0u, 64u, stream));
  if (timing) NDT2D_BATCH_HIP(w, hipEventRecord(w->stage_ev[3], stream));

  // the exact rounds
  const uint32_t chunks = sum_chunks(static_cast<uint32_t>(n_beams));
  const uint32_t threads = static_cast<uint32_t>(std::min<size_t>(kSearchMaxThreads, round_up(T * T, kWave)));
  size_t done = 0, chunk = std::min(kFirstChunk, max_chunk);
  double best_s = 0.0, best_i = kNoIndex;
  while (done < n_jobs)
  {
    const size_t n = std::min(chunk, n_jobs - done);
    launch_exact(chunks, grid.pow2 != 0, static_cast<uint32_t>(n), threads, stream, grid, a, vals_out, static_cast<uint32_t>(done),
                 static_cast<double *>(w->d_partials), evaluated);
    NDT2D_BATCH_HIP(w, hipGetLastError());
    done += n;
    hipLaunchKernelGGL(wide_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream, static_cast<const double *>(w->d_partials),
                       static_cast<uint32_t>(n), w->d_out + 4, keys_out, static_cast<uint32_t>(done), static_cast<uint32_t>(n_jobs),
                       w->d_out);
    NDT2D_BATCH_HIP(w, hipGetLastError());
    NDT2D_BATCH_HIP(w, hipMemcpyAsync(w->h_out, w->d_out, 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
    NDT2D_BATCH_HIP(w, hipStreamSynchronize(stream));
    best_s = w->h_out[0];
    best_i = w->h_out[1];
    const double next_bound = w->h_out[2];
    // strictly below best_sum (1 - 2^-35): nothing left can win or come within the near-tie tolerance
    // (best_sum = 0, no winner yet: never true, the walk goes on)
    const double best_sum = -best_s;
    if (done < n_jobs && next_bound < best_sum * (1.0 - 0x1.0p-35)) break;
    chunk = std::min(chunk * 2, max_chunk);
  }
  if (timing)
  {
    NDT2D_BATCH_HIP(w, hipEventRecord(w->stage_ev[4], stream));
    NDT2D_BATCH_HIP(w, hipStreamSynchronize(stream));
    w->stage_timed = true;
  }
  record_out[0] = best_s;
  record_out[1] = best_s < 0.0 ? best_i : -1.0;   // no candidate scored below 0: no index
  if (stats_out != nullptr)
  {
    stats_out[0] = done;
    stats_out[1] = n_jobs;
  }
  if (bounds_out != nullptr) NDT2D_BATCH_HIP(w, hipMemcpy(bounds_out, keys_in, n_jobs * sizeof(double), hipMemcpyDeviceToHost));
  if (evaluated_out != nullptr) NDT2D_BATCH_HIP(w, hipMemcpy(evaluated_out, evaluated, n_jobs, hipMemcpyDeviceToHost));
  return NDT2D_OK;
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_wide_create(ndt2d_handle h, size_t max_tiles, ndt2d_wide ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || max_tiles == 0 || max_tiles > (size_t(1) << 24)) return NDT2D_ERR_INVALID;
  ndt2d_wide * w = new ndt2d_wide();
  w->h = h;
  w->device = ndt2d_device_id(h);
  w->max_tiles = max_tiles;
  *out = w;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_wide_destroy(ndt2d_wide * w)
{
  NDT2D_C_TRY
  if (w == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::batch_drain(w);
  ndt2d::batch_release(w);
  if (w->d_image != nullptr) (void)hipFree(w->d_image);
  if (w->d_jobs != nullptr) (void)hipFree(w->d_jobs);
  if (w->d_sort_temp != nullptr) (void)hipFree(w->d_sort_temp);
  for (hipEvent_t ev : w->stage_ev)
  {
    if (ev != nullptr) (void)hipEventDestroy(ev);
  }
  delete w;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_wide_last_error(ndt2d_wide * w)
{
  return w != nullptr ? w->err.c_str() : "null wide search";
}

int ndt2d_wide_set_tile(ndt2d_wide * w, uint32_t tile_steps, uint32_t pixels_per_tile)
{
  NDT2D_C_TRY
  if (w == nullptr) return NDT2D_ERR_INVALID;
  if (tile_steps < 1 || tile_steps > ndt2d::wide::kMaxTileSteps)
  {
    return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_set_tile: tile_steps must be 1 .. 32");
  }
  if (pixels_per_tile < 1 || pixels_per_tile > ndt2d::wide::kMaxPixelsPerTile)
  {
    return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_set_tile: pixels_per_tile must be 1 .. 8");
  }
  w->tile_steps = tile_steps;
  w->pixels_per_tile = pixels_per_tile;
  return NDT2D_OK;
  NDT2D_C_CATCH(w)
}

int ndt2d_wide_tile(ndt2d_wide * w, uint32_t * tile_steps, uint32_t * pixels_per_tile)
{
  if (w == nullptr) return NDT2D_ERR_INVALID;
  if (tile_steps != nullptr) *tile_steps = w->tile_steps;
  if (pixels_per_tile != nullptr) *pixels_per_tile = w->pixels_per_tile;
  return NDT2D_OK;
}

int ndt2d_wide_set_timing(ndt2d_wide * w, int enabled)
{
  NDT2D_C_TRY
  if (w == nullptr) return NDT2D_ERR_INVALID;
  if (enabled != 0 && w->stage_ev[0] == nullptr)
  {
    NDT2D_BATCH_HIP(w, hipSetDevice(w->device));
    for (hipEvent_t & ev : w->stage_ev) NDT2D_BATCH_HIP(w, hipEventCreate(&ev));
  }
  w->timing = enabled != 0;
  w->stage_timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(w)
}

int ndt2d_wide_last_ms(ndt2d_wide * w, float * image_ms, float * bounds_ms, float * sort_ms, float * exact_ms)
{
  NDT2D_C_TRY
  if (w == nullptr) return NDT2D_ERR_INVALID;
  if (!w->stage_timed) return batch_fail(w, NDT2D_ERR_STATE, "ndt2d_wide_last_ms: no timed match (ndt2d_wide_set_timing)");
  float * const out[4] = {image_ms, bounds_ms, sort_ms, exact_ms};
  for (int k = 0; k < 4; ++k)
  {
    float ms = 0.0f;
    NDT2D_BATCH_HIP(w, hipEventElapsedTime(&ms, w->stage_ev[k], w->stage_ev[k + 1]));
    if (out[k] != nullptr) *out[k] = ms;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(w)
}

int ndt2d_wide_match(ndt2d_wide * w, const double * pose_xyt, const double * beams_xy, size_t n_beams, const double * dth,
                     size_t n_th, const double * dlin, size_t n_lin, int reuse_image, double * record_out,
                     uint64_t * stats_out, double * bounds_out, uint8_t * evaluated_out)
{
  NDT2D_C_TRY
  if (w == nullptr) return NDT2D_ERR_INVALID;
  if (pose_xyt == nullptr || record_out == nullptr || beams_xy == nullptr || dth == nullptr || dlin == nullptr)
  {
    return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_match: null argument");
  }
  // what ndt2d_set_beams / ndt2d_set_search refuse
  if (n_beams == 0 || n_beams > (1u << 20)) return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_match: bad argument (n_beams)");
  if (n_th == 0 || n_lin == 0 || n_th > (1u << 24) || n_lin > 46340)
  {
    return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_match: bad argument (lattice)");
  }
  if (!std::isfinite(pose_xyt[0]) || !std::isfinite(pose_xyt[1]) || !std::isfinite(pose_xyt[2]))
  {
    return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_match: the pose is not finite");
  }
  // a tile's first candidate must be its lower corner
  for (size_t i = 0; i < n_lin; ++i)
  {
    if (!std::isfinite(dlin[i]) || (i > 0 && !(dlin[i] > dlin[i - 1])))
    {
      return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_match: dlin must be finite and strictly ascending (sort the offsets; "
                                              "ndt2d_search_offsets gives them so)");
    }
  }
  return ndt2d::wide_match(w, pose_xyt, beams_xy, n_beams, dth, n_th, dlin, n_lin, reuse_image, record_out, stats_out, bounds_out,
                           evaluated_out);
  NDT2D_C_CATCH(w)
}

int ndt2d_wide_read_image(ndt2d_wide * w, double * info_out, double * data_out, size_t capacity)
{
  NDT2D_C_TRY
  if (w == nullptr) return NDT2D_ERR_INVALID;
  if (info_out == nullptr) return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_read_image: null argument");
  if (!w->have_image) return batch_fail(w, NDT2D_ERR_STATE, "ndt2d_wide_read_image: no image (ndt2d_wide_match makes one)");
  const ndt2d::wide::Image & im = w->image;
  info_out[0] = im.nx;
  info_out[1] = im.ny;
  info_out[2] = im.origin_x;
  info_out[3] = im.origin_y;
  info_out[4] = im.pitch;
  info_out[5] = im.window;
  info_out[6] = ndt2d::wide::kGuard;
  info_out[7] = 0.0;
  if (data_out == nullptr) return NDT2D_OK;
  const size_t n = static_cast<size_t>(im.nx) * im.ny;
  if (capacity < n) return batch_fail(w, NDT2D_ERR_INVALID, "ndt2d_wide_read_image: capacity below nx * ny pixels");
  NDT2D_BATCH_HIP(w, hipSetDevice(w->device));
  NDT2D_BATCH_HIP(w, hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(w->h))));
  NDT2D_BATCH_HIP(w, hipMemcpy(data_out, w->d_image, n * sizeof(double), hipMemcpyDeviceToHost));
  return NDT2D_OK;
  NDT2D_C_CATCH(w)
}

}  // extern "C"
