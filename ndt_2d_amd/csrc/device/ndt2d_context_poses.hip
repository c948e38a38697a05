// Device layer, pose scoring on a context: batches of poses (from the device, or pipelined from
// host memory), the few-pose path through host-coherent memory, and the particle filter's steps.
#include <algorithm>

#include "device/ndt2d_context.h"

using namespace ndt2d_device;

namespace
{

// angles::normalize_angle / shortest_angular_distance (ROS `angles`)
double normalize_angle(double a)
{
  const double r = std::fmod(a + M_PI, 2.0 * M_PI);
  return r <= 0.0 ? r + M_PI : r - M_PI;
}
double angle_diff(double from, double to) { return normalize_angle(to - from); }

// The per-call part of MotionModel::sample (reference src/motion_model.cpp:48-72):
// decompose the odometry delta and derive the three (mean, sigma) pairs, narrowed
// to float as std::normal_distribution<float> holds them.
ndt2d::MotionParams motion_params(double dx, double dy, double dth, const double * a)
{
  const double trans = std::hypot(dx, dy);
  const double rot1 = (trans > 0.01) ? std::atan2(dy, dx) : 0.0;
  const double rot2 = angle_diff(rot1, dth);
  const double rot1_ = std::min(std::fabs(angle_diff(rot1, 0.0)), std::fabs(angle_diff(rot1, M_PI)));
  const double rot2_ = std::min(std::fabs(angle_diff(rot2, 0.0)), std::fabs(angle_diff(rot2, M_PI)));
  const double sigma_rot1 = std::sqrt(a[0] * rot1_ * rot1_ + a[1] * trans * trans);
  const double sigma_trans =
    std::sqrt(a[2] * trans * trans + a[3] * rot1_ * rot1_ + a[3] * rot2_ * rot2_);
  const double sigma_rot2 = std::sqrt(a[0] * rot2_ * rot2_ + a[1] * trans * trans);
  ndt2d::MotionParams p;
  p.rot1 = static_cast<float>(rot1);
  p.trans = static_cast<float>(trans);
  p.rot2 = static_cast<float>(rot2);
  p.sigma_rot1 = static_cast<float>(sigma_rot1);
  p.sigma_trans = static_cast<float>(sigma_trans);
  p.sigma_rot2 = static_cast<float>(sigma_rot2);
  return p;
}

// A small batch of poses (<= kFewPosesMax) through the block-per-pose kernel: one launch,
// results through host-coherent memory.  arg_beams (optional): the context's new beams,
// handed to the kernel as arguments (<= kArgBeams) -- the caller has made h->beams large
// enough.  stats: the whole of ParticleFilter::measure (normalised weights into h_scores,
// NDT2D_PF_RESULT_DOUBLES into h_out).
int run_few(ndt2d_context * h, const double * arg_beams, size_t n_beams, const double * h_poses,
            size_t n_poses, bool stats, double * h_scores, double * h_out);
// ... and in two steps: the launch, and the wait for its results (one launch may be pending)
int run_few_launch(ndt2d_context * h, const double * arg_beams, size_t n_beams, const double * h_poses,
                   size_t n_poses, bool stats);
int run_few_fetch(ndt2d_context * h, double * h_scores, double * h_out);

}  // namespace

extern "C" {

static int score_poses_launch_impl(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                                   double * d_scores, double * d_stats, bool publish_sums);

int ndt2d_score_poses_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                             double * d_scores, double * d_stats)
{
  NDT2D_C_TRY
  return score_poses_launch_impl(h, d_poses_xyt, n_poses, d_scores, d_stats, false);
  NDT2D_C_CATCH(h)
}

int ndt2d_pose_sums_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses, double * d_scores)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  NDT2D_TEST_MAYBE_FAIL(h, "ndt2d_pose_sums_launch");
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->stats, NDT2D_POSE_STATS_DOUBLES + NDT2D_PF_RESULT_DOUBLES);
  if (rc != NDT2D_OK) return rc;
  if ((rc = ensure_host_res(h)) != NDT2D_OK) return rc;
  return score_poses_launch_impl(h, d_poses_xyt, n_poses, d_scores, h->stats.ptr, true);
  NDT2D_C_CATCH(h)
}

int ndt2d_pose_sums_fetch(ndt2d_handle h, double * sums_out)
{
  NDT2D_C_TRY
  if (h == nullptr || sums_out == nullptr) return NDT2D_ERR_INVALID;
  if (!h->sums_pending) return fail(h, NDT2D_ERR_STATE, "ndt2d_pose_sums_fetch: nothing launched");
  NDT2D_HIP(h, hipSetDevice(h->device));
  h->sums_pending = false;
  const int rc = wait_host_flag(h, kPoseSumsFlagSlot, h->sums_seq, h->sums_pos);
  if (rc != NDT2D_OK) return rc;
  for (int k = 0; k < NDT2D_POSE_STATS_DOUBLES; ++k) sums_out[k] = h->host_res[kPoseSumsSlot + k];
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_finalize_totals_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                                    double * d_weights, const double * totals)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (d_poses_xyt == nullptr || d_weights == nullptr || totals == nullptr || n_poses == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pf_finalize_totals_launch: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->ws_poses, ndt2d::poses_workspace_doubles(n_poses));
  if (rc != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->stats, NDT2D_POSE_STATS_DOUBLES + NDT2D_PF_RESULT_DOUBLES)) != NDT2D_OK) return rc;
  if ((rc = ensure_host_res(h)) != NDT2D_OK) return rc;
  hipError_t e = ndt2d::launch_pf_finalize(d_poses_xyt, n_poses, d_weights, nullptr, totals, h->ws_poses.ptr,
                                           h->stats.ptr + NDT2D_POSE_STATS_DOUBLES,
                                           h->host_res_dev + kPfShardOutSlot, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_pf_finalize");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_result_read(ndt2d_handle h, double * out)
{
  NDT2D_C_TRY
  if (h == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  if (h->host_res == nullptr) return fail(h, NDT2D_ERR_STATE, "ndt2d_pf_result_read: nothing launched");
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  for (int k = 0; k < NDT2D_PF_RESULT_DOUBLES; ++k) out[k] = h->host_res[kPfShardOutSlot + k];
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

static int score_poses_launch_impl(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                                   double * d_scores, double * d_stats, bool publish_sums)
{
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_score_poses_launch: no grid");
  if (h->n_beams == 0) return fail(h, NDT2D_ERR_STATE, "ndt2d_score_poses_launch: set_beams first");
  if (d_poses_xyt == nullptr || d_scores == nullptr || n_poses == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_score_poses_launch: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->ws_poses, ndt2d::poses_workspace_doubles(n_poses));
  if (rc != NDT2D_OK) return rc;

  ndt2d::PosesArgs a{};
  a.grid = h->grid;
  a.beams_xy = h->beams_ptr;
  a.n_beams = static_cast<uint32_t>(h->n_beams);
  a.poses_xyt = d_poses_xyt;
  a.n_poses = n_poses;
  a.scores = d_scores;
  a.beam_rmax = h->beam_rmax;
  {
    // an occupancy bitmap too large for LDS: screen with one bit per block of cells
    const int k = ndt2d::poses_coarse_log2(a, ndt2d::poses_lds_per_block());
    if (k > 0)
    {
      if (h->coarse_log2 != k)
      {
        rc = ensure(h, h->coarse_bits, ndt2d::poses_coarse_words(h->grid, static_cast<uint32_t>(k)) / 2 + 2);
        if (rc != NDT2D_OK) return rc;
        hipError_t ce = ndt2d::poses_coarse_bits_launch(h->grid, static_cast<uint32_t>(k),
                                                        reinterpret_cast<uint32_t *>(h->coarse_bits.ptr), h->stream);
        if (ce != hipSuccess) return fail_hip(h, ce, "poses_coarse_bits_launch");
        h->coarse_log2 = k;
      }
      a.coarse_bits = reinterpret_cast<const uint32_t *>(h->coarse_bits.ptr);
      a.coarse_log2 = static_cast<uint32_t>(k);
    }
  }

  ndt2d::LaunchInfo info{"", 0};
  if (h->timing)
  {
    if (int trc = next_timing_slot(h); trc != NDT2D_OK) return trc;
    NDT2D_HIP(h, hipEventRecord(h->ev0, h->stream));
  }
  unsigned long long sums_seq = 0;
  if (publish_sums)
  {
    sums_seq = ++h->seq;
    h->sums_pos = h->queued;
  }
  hipError_t e = ndt2d::launch_score_poses(a, h->ws_poses.ptr, d_stats, h->force_variant,
                                           h->stream, h->timing ? h->ev1 : nullptr, &info,
                                           publish_sums ? h->host_res_dev + kPoseSumsSlot : nullptr, sums_seq);
  if (e != hipSuccess) return fail_hip(h, e, "launch_score_poses");
  if (publish_sums)
  {
    h->sums_seq = sums_seq;
    h->sums_pending = true;
  }
  h->timed = h->timing;
  h->last_kernels = info.n_kernels;
  h->last_variant = info.variant;
  return NDT2D_OK;
}

int ndt2d_score_poses_beams(ndt2d_handle h, const double * beams_xy, size_t n_beams,
                            const double * h_poses_xyt, size_t n_poses, double * h_scores)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (beams_xy == nullptr || n_beams == 0 || n_beams > (1u << 20) || h_poses_xyt == nullptr ||
      h_scores == nullptr || n_poses == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_score_poses_beams: bad argument");
  }
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_score_poses_beams: no grid");
  NDT2D_HIP(h, hipSetDevice(h->device));
  if (n_poses <= ndt2d::kFewPoses && n_beams <= ndt2d::kArgBeams &&
      h->force_variant == ndt2d::kVariantAuto && !h->batched_only)
  {
    // beams AND poses as kernel arguments: one launch, no copy; the kernel leaves the beams
    // in the context's beam buffer for the calls that follow on this scan
    int rc = ensure(h, h->beams, 2 * n_beams + 2);
    if (rc != NDT2D_OK) return rc;
    ndt2d::PosesArgs probe{};
    probe.n_beams = static_cast<uint32_t>(n_beams);
    probe.n_poses = n_poses;
    if (ndt2d::score_few_supported(probe, 64 * 1024))
    {
      // the kernel overwrites the context's beam buffer: until it has reported back the
      // context holds no beams (a failed wait must not leave new beams under the old
      // count and reach)
      h->n_beams = 0;
      h->beams_ptr = nullptr;
      h->has_search = false;
      rc = run_few(h, beams_xy, n_beams, h_poses_xyt, n_poses, false, h_scores, nullptr);
      if (rc != NDT2D_OK) return rc;
      h->n_beams = n_beams;
      h->beams_ptr = h->beams.ptr;
      h->has_search = false;   // see ndt2d_set_beams
      h->beam_rmax = beam_reach(beams_xy, n_beams);
      return NDT2D_OK;
    }
  }
  int rc = ndt2d_set_beams(h, beams_xy, n_beams);
  if (rc != NDT2D_OK) return rc;
  return ndt2d_score_poses(h, h_poses_xyt, n_poses, h_scores, nullptr);
  NDT2D_C_CATCH(h)
}

int ndt2d_score_poses_beams_launch(ndt2d_handle h, const double * beams_xy, size_t n_beams,
                                   const double * h_poses_xyt, size_t n_poses)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (h_poses_xyt == nullptr || n_poses == 0 || (beams_xy != nullptr && n_beams == 0))
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_score_poses_beams_launch: bad argument");
  }
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_score_poses_beams_launch: no grid");
  if (beams_xy == nullptr) n_beams = h->n_beams;
  ndt2d::PosesArgs probe{};
  probe.n_beams = static_cast<uint32_t>(n_beams);
  probe.n_poses = n_poses;
  // only what travels as kernel arguments: nothing of the caller's is read after the return
  if (n_poses > ndt2d::kFewPoses || n_beams == 0 || (beams_xy != nullptr && n_beams > ndt2d::kArgBeams) ||
      h->force_variant != ndt2d::kVariantAuto || h->batched_only || !ndt2d::score_few_supported(probe, 64 * 1024))
  {
    return fail(h, NDT2D_ERR_STATE, "ndt2d_score_poses_beams_launch: not a kernel-argument launch (use ndt2d_score_poses_beams)");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  if (beams_xy == nullptr) return run_few_launch(h, nullptr, n_beams, h_poses_xyt, n_poses, false);
  int rc = ensure(h, h->beams, 2 * n_beams + 2);
  if (rc != NDT2D_OK) return rc;
  h->n_beams = 0;
  h->beams_ptr = nullptr;
  h->has_search = false;
  rc = run_few_launch(h, beams_xy, n_beams, h_poses_xyt, n_poses, false);
  if (rc != NDT2D_OK) return rc;
  // (the kernel is queued: what follows on the stream finds the beams in place; a failed
  // ndt2d_score_fetch takes them away again)
  h->n_beams = n_beams;
  h->beams_ptr = h->beams.ptr;
  h->beam_rmax = beam_reach(beams_xy, n_beams);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_score_fetch(ndt2d_handle h, double * h_scores)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (h_scores == nullptr) return fail(h, NDT2D_ERR_INVALID, "ndt2d_score_fetch: bad argument");
  const int rc = run_few_fetch(h, h_scores, nullptr);
  if (rc != NDT2D_OK && rc != NDT2D_ERR_STATE)
  {
    h->n_beams = 0;
    h->beams_ptr = nullptr;
    h->has_search = false;
  }
  return rc;
  NDT2D_C_CATCH(h)
}

// A LARGE batch of poses from (pageable or pinned) host memory -- ParticleFilter::measure of a
// big filter through the drop-in boundary (reference src/particle_filter.cpp:78-89; BASELINE
// configs[4]: 10^6 particles = 24 MB in, 8 MB out): the batch is cut into pieces, piece k + 1 is
// uploaded on a stream of its own while piece k is scored, and (scores only) piece k - 1 travels
// back on a third.  Sharding a pose set leaves every raw score bit-identical (a lane's score
// does not depend on the launch geometry), the pieces' moment sums are added in piece order.
//   measure: weights = scores normalised by the total, h_out = the statistics (updateStatistics)
//   else:    h_scores = raw scores, h_stats (optional) = the eight moment sums
constexpr size_t kPipelineFromPoses = 1u << 17;   // 3 MB of poses: below, the pieces cost more than they hide

static int pipeline_pieces_for(const ndt2d_context * h, size_t n_poses)
{
  if (h->pipeline_pieces == 1 || n_poses < kPipelineFromPoses) return 1;
  int pieces = h->pipeline_pieces > 0 ? h->pipeline_pieces : 4;
  // (no piece below a quarter of the threshold)
  while (pieces > 1 && n_poses / static_cast<size_t>(pieces) < kPipelineFromPoses / 4) --pieces;
  return pieces > NDT2D_PIPELINE_PIECES ? NDT2D_PIPELINE_PIECES : pieces;
}

static int pipelined_pose_batch(ndt2d_context * h, const double * h_poses_xyt, size_t n_poses, int pieces,
                                bool measure, double * h_scores, double * h_stats_or_out)
{
  int rc = ensure(h, h->tmp_poses, 3 * n_poses);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->tmp_scores, n_poses);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->stats, NDT2D_POSE_STATS_DOUBLES + NDT2D_PF_RESULT_DOUBLES);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->piece_stats, static_cast<size_t>(NDT2D_PIPELINE_PIECES) * NDT2D_POSE_STATS_DOUBLES);
  if (rc != NDT2D_OK) return rc;
  if (h->up_stream == nullptr) NDT2D_HIP(h, hipStreamCreateWithFlags(&h->up_stream, hipStreamNonBlocking));
  if (h->down_stream == nullptr) NDT2D_HIP(h, hipStreamCreateWithFlags(&h->down_stream, hipStreamNonBlocking));
  if (h->pipe_idle == nullptr) NDT2D_HIP(h, hipEventCreateWithFlags(&h->pipe_idle, hipEventDisableTiming));
  for (int k = 0; k < pieces; ++k)
  {
    if (h->pipe_up[k] == nullptr) NDT2D_HIP(h, hipEventCreateWithFlags(&h->pipe_up[k], hipEventDisableTiming));
    if (h->pipe_scored[k] == nullptr) NDT2D_HIP(h, hipEventCreateWithFlags(&h->pipe_scored[k], hipEventDisableTiming));
  }
  // Whatever fails from here on, nothing of this call may still be reading the caller's poses
  // or writing the caller's scores when it returns.
  auto drain = [&](int code) -> int {
    (void)hipStreamSynchronize(h->up_stream);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(h->down_stream);
    return code;
  };
  // (what the main stream still has queued may read the staging buffers: the uploads wait for it)
  NDT2D_HIP(h, hipEventRecord(h->pipe_idle, h->stream));
  NDT2D_HIP(h, hipStreamWaitEvent(h->up_stream, h->pipe_idle, 0));
  const bool want_sums = measure || h_stats_or_out != nullptr;
  // Equal pieces of whole groups of 64 poses.  (A smaller first piece -- nothing runs under its
  // upload -- was measured and lost: the batched kernel's blocks walk their groups in rounds, and
  // pieces of 1/7 and 2/7 of cfg-5 fall between two round counts, 240 us for what should take 165.)
  // No event pairs around the pieces' kernels (ndt2d_launch_history_ms): a pair costs the stream
  // 11 us per piece.
  const size_t unit = ((n_poses + static_cast<size_t>(pieces) - 1) / static_cast<size_t>(pieces) + 63) / 64 * 64;
  const bool timing_was = h->timing;
  h->timing = false;
  auto finish = [&](int code) -> int {
    h->timing = timing_was;
    return code == NDT2D_OK ? code : drain(code);
  };
  int n_pieces = 0;
  hipError_t e = hipSuccess;
  size_t prev_off = 0, prev_cnt = 0;
  // raw scores: piece k - 1 travels back once piece k has been queued behind it (a download
  // into ordinary host memory holds the calling thread until the piece has been scored)
  auto download = [&](size_t off, size_t cnt, int k) -> hipError_t {
    hipError_t de = hipStreamWaitEvent(h->down_stream, h->pipe_scored[k], 0);
    if (de == hipSuccess)
    {
      de = hipMemcpyAsync(h_scores + off, h->tmp_scores.ptr + off, cnt * sizeof(double), hipMemcpyDeviceToHost,
                          h->down_stream);
    }
    return de;
  };
  for (size_t off = 0; off < n_poses; ++n_pieces)
  {
    const size_t cnt = n_poses - off < unit ? n_poses - off : unit;
    const int k = n_pieces;
    e = hipMemcpyAsync(h->tmp_poses.ptr + 3 * off, h_poses_xyt + 3 * off, 3 * cnt * sizeof(double),
                       hipMemcpyHostToDevice, h->up_stream);
    if (e == hipSuccess) e = hipEventRecord(h->pipe_up[k], h->up_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->pipe_up[k], 0);
    if (e != hipSuccess) return finish(fail_hip(h, e, "pipelined_pose_batch: upload"));
    rc = score_poses_launch_impl(h, h->tmp_poses.ptr + 3 * off, cnt, h->tmp_scores.ptr + off,
                                 want_sums ? h->piece_stats.ptr + static_cast<size_t>(k) * NDT2D_POSE_STATS_DOUBLES : nullptr,
                                 false);
    if (rc != NDT2D_OK) return finish(rc);
    if (!measure)
    {
      e = hipEventRecord(h->pipe_scored[k], h->stream);
      if (e == hipSuccess && k > 0) e = download(prev_off, prev_cnt, k - 1);
      if (e != hipSuccess) return finish(fail_hip(h, e, "pipelined_pose_batch: download"));
      prev_off = off;
      prev_cnt = cnt;
    }
    off += cnt;
  }
  if (!measure)
  {
    e = download(prev_off, prev_cnt, n_pieces - 1);
    if (e != hipSuccess) return finish(fail_hip(h, e, "pipelined_pose_batch: download"));
  }
  if (want_sums)
  {
    e = ndt2d::launch_sum_moment_rows(h->piece_stats.ptr, static_cast<uint32_t>(n_pieces), h->stats.ptr, h->stream);
    if (e != hipSuccess) return finish(fail_hip(h, e, "launch_sum_moment_rows"));
  }
  if (measure)
  {
    double * d_out = h->stats.ptr + NDT2D_POSE_STATS_DOUBLES;
    rc = ndt2d_pf_finalize_launch(h, h->tmp_poses.ptr, n_poses, h->tmp_scores.ptr, h->stats.ptr, d_out);
    if (rc != NDT2D_OK) return finish(rc);
    e = hipMemcpyAsync(h_scores, h->tmp_scores.ptr, n_poses * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
    {
      e = hipMemcpyAsync(h_stats_or_out, d_out, NDT2D_PF_RESULT_DOUBLES * sizeof(double), hipMemcpyDeviceToHost,
                         h->stream);
    }
  }
  else if (h_stats_or_out != nullptr)
  {
    e = hipMemcpyAsync(h_stats_or_out, h->stats.ptr, NDT2D_POSE_STATS_DOUBLES * sizeof(double),
                       hipMemcpyDeviceToHost, h->stream);
  }
  if (e != hipSuccess) return finish(fail_hip(h, e, "pipelined_pose_batch: results"));
  e = hipStreamSynchronize(h->down_stream);
  if (e != hipSuccess) return finish(fail_hip(h, e, "hipStreamSynchronize"));
  {
    const uint64_t q_ = h->queued;
    e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return finish(fail_hip(h, e, "hipStreamSynchronize"));
    if (h->reached < q_) h->reached = q_;
  }
  h->timing = timing_was;
  h->last_pieces = n_pieces;
  return NDT2D_OK;
}

int ndt2d_score_poses(ndt2d_handle h, const double * h_poses_xyt, size_t n_poses,
                      double * h_scores, double * h_stats)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (h_poses_xyt == nullptr || h_scores == nullptr || n_poses == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_score_poses: bad argument");
  }
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_score_poses: no grid");
  if (h->n_beams == 0) return fail(h, NDT2D_ERR_STATE, "ndt2d_score_poses: set_beams first");
  NDT2D_HIP(h, hipSetDevice(h->device));
  h->last_pieces = 1;
  int rc;

  // A small batch (scorePoints / scoreScan: ONE pose; a particle filter of the node's
  // default size: <= 500): a block per pose and a thread per beam, the poses as kernel
  // arguments (<= 8) or through one staged copy, the scores written straight into
  // host-coherent memory behind a flag the host spins on -- one launch.
  if (h_stats == nullptr && n_poses <= ndt2d::kFewPosesMax &&
      h->force_variant == ndt2d::kVariantAuto && !h->batched_only)
  {
    ndt2d::PosesArgs probe{};
    probe.n_beams = static_cast<uint32_t>(h->n_beams);
    probe.n_poses = n_poses;
    if (ndt2d::score_few_supported(probe, 64 * 1024))
    {
      return run_few(h, nullptr, h->n_beams, h_poses_xyt, n_poses, false, h_scores, nullptr);
    }
  }

  rc = ensure(h, h->stats, NDT2D_POSE_STATS_DOUBLES);
  if (rc != NDT2D_OK) return rc;
  // Pinned host memory (ndt2d_host_alloc) is addressed by the kernels directly: the
  // poses are read over PCIe once, the scores written once, no copy is queued.
  const double * d_poses = device_view(h_poses_xyt);
  double * d_scores = device_view(h_scores);
  if (d_poses == nullptr && d_scores == nullptr)
  {
    // a large batch from ordinary host memory: uploads, scoring and downloads piece by piece, overlapped
    const int pieces = pipeline_pieces_for(h, n_poses);
    if (pieces > 1) return pipelined_pose_batch(h, h_poses_xyt, n_poses, pieces, false, h_scores, h_stats);
  }
  if (d_poses == nullptr)
  {
    rc = ensure(h, h->tmp_poses, 3 * n_poses);
    if (rc != NDT2D_OK) return rc;
    NDT2D_HIP(h, hipMemcpyAsync(h->tmp_poses.ptr, h_poses_xyt, 3 * n_poses * sizeof(double),
                                hipMemcpyHostToDevice, h->stream));
    d_poses = h->tmp_poses.ptr;
  }
  const bool copy_scores = d_scores == nullptr;
  if (copy_scores)
  {
    rc = ensure(h, h->tmp_scores, n_poses);
    if (rc != NDT2D_OK) return rc;
    d_scores = h->tmp_scores.ptr;
  }
  rc = ndt2d_score_poses_launch(h, d_poses, n_poses, d_scores, h_stats != nullptr ? h->stats.ptr : nullptr);
  if (rc != NDT2D_OK) return rc;
  if (copy_scores)
  {
    NDT2D_HIP(h, hipMemcpyAsync(h_scores, d_scores, n_poses * sizeof(double), hipMemcpyDeviceToHost,
                                h->stream));
  }
  if (h_stats != nullptr)
  {
    NDT2D_HIP(h, hipMemcpyAsync(h_stats, h->stats.ptr, NDT2D_POSE_STATS_DOUBLES * sizeof(double),
                                hipMemcpyDeviceToHost, h->stream));
  }
  NDT2D_SYNC(h);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_finalize_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                             double * d_weights, const double * d_stats, double * d_out)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (d_poses_xyt == nullptr || d_weights == nullptr || d_stats == nullptr || d_out == nullptr ||
      n_poses == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pf_finalize_launch: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->ws_poses, ndt2d::poses_workspace_doubles(n_poses));
  if (rc != NDT2D_OK) return rc;
  hipError_t e = ndt2d::launch_pf_finalize(d_poses_xyt, n_poses, d_weights, d_stats, nullptr,
                                           h->ws_poses.ptr, d_out, nullptr, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_pf_finalize");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_measure(ndt2d_handle h, const double * h_poses_xyt, size_t n_poses,
                     double * h_weights, double * h_out)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (h_poses_xyt == nullptr || h_weights == nullptr || h_out == nullptr || n_poses == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pf_measure: bad argument");
  }
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_pf_measure: no grid");
  if (h->n_beams == 0) return fail(h, NDT2D_ERR_STATE, "ndt2d_pf_measure: set_beams first");
  NDT2D_HIP(h, hipSetDevice(h->device));
  h->last_pieces = 1;
  if (n_poses <= ndt2d::kFewPosesMax && h->force_variant == ndt2d::kVariantAuto && !h->batched_only)
  {
    // a filter of the node's size (<= 500 particles by default): scoring and
    // updateStatistics in ONE launch, weights and result through host-coherent memory
    ndt2d::PosesArgs probe{};
    probe.n_beams = static_cast<uint32_t>(h->n_beams);
    probe.n_poses = n_poses;
    if (ndt2d::score_few_supported(probe, 64 * 1024))
    {
      return run_few(h, nullptr, h->n_beams, h_poses_xyt, n_poses, true, h_weights, h_out);
    }
  }
  {
    // a large filter: the particles go up piece by piece under the scoring of the piece before
    const int pieces = pipeline_pieces_for(h, n_poses);
    if (pieces > 1) return pipelined_pose_batch(h, h_poses_xyt, n_poses, pieces, true, h_weights, h_out);
  }
  int rc = ensure(h, h->tmp_poses, 3 * n_poses);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->tmp_scores, n_poses);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->stats, NDT2D_POSE_STATS_DOUBLES + NDT2D_PF_RESULT_DOUBLES);
  if (rc != NDT2D_OK) return rc;
  NDT2D_HIP(h, hipMemcpyAsync(h->tmp_poses.ptr, h_poses_xyt, 3 * n_poses * sizeof(double),
                              hipMemcpyHostToDevice, h->stream));
  rc = ndt2d_score_poses_launch(h, h->tmp_poses.ptr, n_poses, h->tmp_scores.ptr, h->stats.ptr);
  if (rc != NDT2D_OK) return rc;
  double * d_out = h->stats.ptr + NDT2D_POSE_STATS_DOUBLES;
  rc = ndt2d_pf_finalize_launch(h, h->tmp_poses.ptr, n_poses, h->tmp_scores.ptr, h->stats.ptr, d_out);
  if (rc != NDT2D_OK) return rc;
  NDT2D_HIP(h, hipMemcpyAsync(h_weights, h->tmp_scores.ptr, n_poses * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
  NDT2D_HIP(h, hipMemcpyAsync(h_out, d_out, NDT2D_PF_RESULT_DOUBLES * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
  NDT2D_SYNC(h);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_noise_launch(ndt2d_handle h, uint64_t seed, uint64_t step, uint64_t first_index,
                          size_t n, float * d_noise_out)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (d_noise_out == nullptr || n == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pf_noise_launch: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  hipError_t e = ndt2d::launch_pf_noise(d_noise_out, n, seed, first_index, step, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_pf_noise");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_motion_launch(ndt2d_handle h, double * d_poses_xyt, size_t n, double dx, double dy,
                           double dth, const double * alphas5, const float * d_noise,
                           uint64_t seed, uint64_t step, uint64_t first_index)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (d_poses_xyt == nullptr || alphas5 == nullptr || n == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pf_motion_launch: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  const ndt2d::MotionParams p = motion_params(dx, dy, dth, alphas5);
  hipError_t e =
    ndt2d::launch_pf_motion(d_poses_xyt, n, p, d_noise, seed, first_index, step, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_pf_motion");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_init_launch(ndt2d_handle h, double * d_poses_xyt, size_t n, double x, double y,
                         double theta, double sigma_x, double sigma_y, double sigma_theta,
                         const float * d_noise, uint64_t seed, uint64_t step,
                         uint64_t first_index)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (d_poses_xyt == nullptr || n == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pf_init_launch: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  ndt2d::InitParams p;
  p.x = static_cast<float>(x);
  p.y = static_cast<float>(y);
  p.theta = static_cast<float>(theta);
  p.sigma_x = static_cast<float>(sigma_x);
  p.sigma_y = static_cast<float>(sigma_y);
  p.sigma_theta = static_cast<float>(sigma_theta);
  hipError_t e =
    ndt2d::launch_pf_init(d_poses_xyt, n, p, d_noise, seed, first_index, step, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_pf_init");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pose_moments_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n,
                              const double * d_weights, double * d_stats)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (d_poses_xyt == nullptr || d_stats == nullptr || n == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pose_moments_launch: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->ws_poses, ndt2d::poses_workspace_doubles(n));
  if (rc != NDT2D_OK) return rc;
  hipError_t e =
    ndt2d::launch_pose_moments(d_poses_xyt, n, d_weights, h->ws_poses.ptr, d_stats, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_pose_moments");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_pf_update(ndt2d_handle h, double * h_poses_xyt, size_t n, double dx, double dy,
                    double dth, const double * alphas5, const float * h_noise, uint64_t seed,
                    uint64_t step, double * h_weights, double * h_out)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (h_poses_xyt == nullptr || alphas5 == nullptr || h_weights == nullptr || h_out == nullptr ||
      n == 0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_pf_update: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->tmp_poses, 3 * n);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->tmp_scores, n);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->stats, NDT2D_POSE_STATS_DOUBLES + NDT2D_PF_RESULT_DOUBLES);
  if (rc != NDT2D_OK) return rc;
  const float * d_noise = nullptr;
  if (h_noise != nullptr)
  {
    rc = ensure(h, h->tmp_noise, (3 * n * sizeof(float) + sizeof(double) - 1) / sizeof(double));
    if (rc != NDT2D_OK) return rc;
    NDT2D_HIP(h, hipMemcpyAsync(h->tmp_noise.ptr, h_noise, 3 * n * sizeof(float),
                                hipMemcpyHostToDevice, h->stream));
    d_noise = reinterpret_cast<const float *>(h->tmp_noise.ptr);
  }
  NDT2D_HIP(h, hipMemcpyAsync(h->tmp_poses.ptr, h_poses_xyt, 3 * n * sizeof(double),
                              hipMemcpyHostToDevice, h->stream));
  NDT2D_HIP(h, hipMemcpyAsync(h->tmp_scores.ptr, h_weights, n * sizeof(double),
                              hipMemcpyHostToDevice, h->stream));
  rc = ndt2d_pf_motion_launch(h, h->tmp_poses.ptr, n, dx, dy, dth, alphas5, d_noise, seed, step, 0);
  if (rc != NDT2D_OK) return rc;
  rc = ndt2d_pose_moments_launch(h, h->tmp_poses.ptr, n, h->tmp_scores.ptr, h->stats.ptr);
  if (rc != NDT2D_OK) return rc;
  double * d_out = h->stats.ptr + NDT2D_POSE_STATS_DOUBLES;
  rc = ndt2d_pf_finalize_launch(h, h->tmp_poses.ptr, n, h->tmp_scores.ptr, h->stats.ptr, d_out);
  if (rc != NDT2D_OK) return rc;
  NDT2D_HIP(h, hipMemcpyAsync(h_poses_xyt, h->tmp_poses.ptr, 3 * n * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
  NDT2D_HIP(h, hipMemcpyAsync(h_weights, h->tmp_scores.ptr, n * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
  NDT2D_HIP(h, hipMemcpyAsync(h_out, d_out, NDT2D_PF_RESULT_DOUBLES * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
  NDT2D_SYNC(h);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

}  // extern "C"

namespace
{

// The results of the pending few-pose launch: wait for its flag, copy them out.
int run_few_fetch(ndt2d_context * h, double * h_scores, double * h_out)
{
  if (!h->few_pending) return fail(h, NDT2D_ERR_STATE, "no few-pose launch is pending");
  h->few_pending = false;
  const int rc = wait_host_flag(h, kScoreFlagSlot, h->few_seq, h->few_pos);
  if (rc != NDT2D_OK) return rc;
  if (h_scores != nullptr) std::memcpy(h_scores, h->host_res + kScoreSlot, h->few_n_poses * sizeof(double));
  if (h->few_stats && h_out != nullptr)
  {
    for (int k = 0; k < NDT2D_PF_RESULT_DOUBLES; ++k) h_out[k] = h->host_res[kPfOutSlot + k];
  }
  return NDT2D_OK;
}

int run_few_launch(ndt2d_context * h, const double * arg_beams, size_t n_beams, const double * h_poses,
                   size_t n_poses, bool stats)
{
  if (h->few_pending)
  {
    // (results nobody collected: the slots are about to be written again)
    const int drc = run_few_fetch(h, nullptr, nullptr);
    if (drc != NDT2D_OK) return drc;
  }

  int rc = ensure_host_res(h);
  if (rc != NDT2D_OK) return rc;
  ndt2d::PosesArgs a{};
  a.grid = h->grid;
  a.beams_xy = arg_beams != nullptr ? h->beams.ptr : h->beams_ptr;
  a.n_beams = static_cast<uint32_t>(n_beams);
  a.n_poses = n_poses;
  a.scores = h->host_res_dev + kScoreSlot;
  ndt2d::FewPoses few{};
  bool poses_in_place = false;
  if (n_poses <= ndt2d::kFewPoses)
  {
    std::memcpy(few.xyt, h_poses, 3 * n_poses * sizeof(double));
    a.poses_xyt = nullptr;
  }
  else
  {
    // through the pinned staging buffer, which the kernel reads in place over PCIe (24 bytes
    // per block): no copy command, no event; the call returns after the kernel has finished,
    // so the buffer is free for the next one (the caller's buffer is free on return)
    if ((rc = ensure(h, h->tmp_poses, 3 * n_poses)) != NDT2D_OK) return rc;
    if ((rc = stage_acquire(h, h->stage_call, 3 * n_poses)) != NDT2D_OK) return rc;
    std::memcpy(h->stage_call.ptr, h_poses, 3 * n_poses * sizeof(double));
    if (h->stage_call.dev != nullptr)
    {
      a.poses_xyt = h->stage_call.dev;
      poses_in_place = true;
    }
    else
    {
      if ((rc = stage_submit(h, h->stage_call, h->tmp_poses.ptr, 3 * n_poses)) != NDT2D_OK) return rc;
      a.poses_xyt = h->tmp_poses.ptr;
    }
  }
  ndt2d::FewOut out{};
  out.flag = reinterpret_cast<unsigned long long *>(h->host_res_dev + kScoreFlagSlot);
  out.seq = ++h->seq;
  out.done = h->done_words;
  out.beams_out = arg_beams != nullptr ? h->beams.ptr : nullptr;
  out.stats = stats ? 1 : 0;
  if (stats)
  {
    if ((rc = ensure(h, h->tmp_scores, n_poses)) != NDT2D_OK) return rc;
    out.dev_scores = h->tmp_scores.ptr;
    out.host_out = h->host_res_dev + kPfOutSlot;
    out.dev_poses = poses_in_place ? h->tmp_poses.ptr : nullptr;
  }
  out.side = h->bytes_job;   // (n == 0: none)
  hipError_t e = ndt2d::launch_score_few(a, &few, out, arg_beams, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_score_few");
  // the kernel reads the staged poses in place: the buffer is its until it has finished
  if (poses_in_place && (rc = stage_mark(h, h->stage_call)) != NDT2D_OK) return rc;
  // (every mark so far is behind this kernel or behind work queued before it: its flag proves them all)
  const uint64_t flag_pos = h->queued;
  h->bytes_job.n = 0;
  h->timed = false;
  h->last_kernels = 1;
  h->last_variant = h->grid.pow2 ? "poses/block-per-pose/pow2" : "poses/block-per-pose/div";
  h->few_pending = true;
  h->few_seq = out.seq;
  h->few_pos = flag_pos;
  h->few_n_poses = n_poses;
  h->few_stats = stats;
  return NDT2D_OK;
}

int run_few(ndt2d_context * h, const double * arg_beams, size_t n_beams, const double * h_poses,
            size_t n_poses, bool stats, double * h_scores, double * h_out)
{
  const int rc = run_few_launch(h, arg_beams, n_beams, h_poses, n_poses, stats);
  return rc != NDT2D_OK ? rc : run_few_fetch(h, h_scores, h_out);
}

}  // namespace
