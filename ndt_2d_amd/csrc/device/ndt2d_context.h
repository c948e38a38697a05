// The device layer's context (include/ndt2d_hip.h, section 1): one per (plugin instance, GPU),
// holding the HBM-resident NDT grid, beams and search tables and the stream the kernels of
// ndt2d_kernels.h are launched on -- and the small helpers every unit of csrc/device/ needs.
// Private to csrc/device/: the modules beside the context talk to it through the C ABI.
#ifndef NDT2D_CONTEXT_H_
#define NDT2D_CONTEXT_H_

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "ndt2d_kernels.h"

// (nothing below is for the library's dynamic symbol table)
#pragma GCC visibility push(hidden)

// Both buffer types own their memory: a context's buffers go with it (ndt2d_destroy); assigning
// an empty one frees early.
struct DeviceBuffer
{
  double * ptr = nullptr;
  size_t cap = 0;  // doubles
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer & operator=(const DeviceBuffer &) = delete;
  DeviceBuffer(DeviceBuffer && o) noexcept { *this = std::move(o); }
  // (what this one held goes with `o`)
  DeviceBuffer & operator=(DeviceBuffer && o) noexcept { std::swap(ptr, o.ptr); std::swap(cap, o.cap); return *this; }
  ~DeviceBuffer() { if (ptr != nullptr) (void)hipFree(ptr); }
};

// Pinned host staging for small uploads: the copy is truly asynchronous and the
// caller's buffer is free as soon as the call returns.
struct PinnedStage
{
  double * ptr = nullptr;
  double * dev = nullptr;   // the same memory as the device addresses it (kernels may read it in place)
  size_t cap = 0;  // doubles
  // the stream position (ndt2d_context::queued) behind the buffer's last queued reader: the
  // buffer may be written again once the stream is known to have passed it
  bool pending = false;
  uint64_t needed = 0;
  PinnedStage() = default;
  PinnedStage(const PinnedStage &) = delete;
  PinnedStage & operator=(const PinnedStage &) = delete;
  PinnedStage(PinnedStage && o) noexcept { *this = std::move(o); }
  PinnedStage & operator=(PinnedStage && o) noexcept
  {
    std::swap(ptr, o.ptr), std::swap(dev, o.dev), std::swap(cap, o.cap);
    std::swap(pending, o.pending), std::swap(needed, o.needed);
    return *this;
  }
  ~PinnedStage() { if (ptr != nullptr) (void)hipHostFree(ptr); }
};

// Pieces a large pose batch from host memory is cut into (see pipelined_pose_batch)
#define NDT2D_PIPELINE_PIECES 16

struct ndt2d_context
{
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;

  bool has_grid = false;
  ndt2d::GridDesc grid{};
  DeviceBuffer cells_lds_image;
  DeviceBuffer cells_global;
  DeviceBuffer occ_bits;  // uint32 words stored in a double buffer
  DeviceBuffer cell_bytes;  // per-cell occupancy-map bytes of the extended grid
  // what a list install left to do (bytes_job.n > 0): the map bytes around the listed cells.
  // Only the small-lattice search reads them: the job rides along in the next few-pose launch
  // (the mapper's scoreScan) or runs ahead of the next search, whichever comes first.
  ndt2d::SparseBytesJob bytes_job{};
  // ndt2d_grid_stage_begin ... _commit: capacity (0: none open) and grid size of the open list
  size_t stage_cap = 0;
  uint32_t stage_sx = 0, stage_sy = 0;
  bool stage_may_compact = false;
  DeviceBuffer compact;     // [cells6 | compact records | cell ranks]: ndt2d_set_grid's upload
  DeviceBuffer cells6;    // raw {mean, information, n} records of a device-built grid
  const double * cells6_ptr = nullptr;  // ... of the installed grid, wherever they live
  // a grid installed as the list of its touched cells (ndt2d_set_grid_sparse): the list on the
  // device (inside `compact`), from which ndt2d_get_grid makes the dense records on demand
  DeviceBuffer ranks;       // cell -> compact record table of such a grid (uint16 per cell)
  // particle scoring on a grid whose occupancy bitmap does not fit LDS: one bit per block of
  // cells, made from the bitmap on the first launch that needs it (-1: not made for this grid)
  DeviceBuffer coarse_bits;
  int coarse_log2 = -1;
  // ... and the small-lattice search on a window wider than 256 cells: map bytes per block of cells
  DeviceBuffer block_bytes;
  int block_bytes_log2 = -1;
  uint32_t sparse_n = 0;
  const uint32_t * sparse_index = nullptr;
  const double * sparse_cells6 = nullptr;
  // device NDT build scratch + host staging that must outlive the async copies
  DeviceBuffer b_points, b_scans, b_offsets, b_world, b_keys, b_vals, b_temp, b_seg;
  std::vector<double> stage_scans;
  std::vector<uint32_t> stage_offsets;
  std::vector<uint32_t> stage_seen;   // list install: one bit per cell already listed

  DeviceBuffer beams;
  size_t n_beams = 0;
  PinnedStage stage_beams, stage_tables, stage_grid, stage_call;
  // where the launches read beams and tables: the buffers of ndt2d_set_beams /
  // ndt2d_set_search, or one buffer filled by a single copy (ndt2d_set_search_beams)
  const double * beams_ptr = nullptr;
  const double * tables_ptr = nullptr;
  DeviceBuffer call_dev;

  // Results of small calls go straight into host-coherent pinned memory, followed by a
  // sequence number the host spins on (a stream synchronisation costs ~4 us more):
  //   [0..11] match record   [16] match flag   [24] score flag   [32..2079] scores / weights
  //   [2080..2087] particle statistics
  // Stream positions: `queued` counts the marks handed out behind queued work
  // (stage_mark), `reached` is the newest mark the in-order stream is known to have
  // passed -- a result flag seen by the host proves everything queued before that kernel done.
  uint64_t queued = 0, reached = 0;
  uint64_t match_pos = 0, few_pos = 0;   // `queued` when the pending search / few-pose launch went out
  double * host_res = nullptr;      // host address
  double * host_res_dev = nullptr;  // the same memory as the GPU addresses it
  unsigned long long seq = 0;       // last sequence number handed out
  unsigned long long match_seq = 0; // ... to the pending match launch
  unsigned long long * done_words = nullptr;   // score_few launches: one word per pose

  DeviceBuffer tables;  // dth | cos | sin | dlin
  // ndt2d_set_search keeps the tables in its pinned staging buffer and leaves the upload
  // to the launch: the small-lattice search takes them as kernel arguments (no copy)
  bool tables_uploaded = false;
  size_t n_th = 0, n_lin = 0;
  double pose_x = 0.0, pose_y = 0.0;
  double dlin_absmax = 0.0;
  double patch_span = -1.0;   // see MatchArgs::patch_span
  double strip_span_long = 0.0, strip_span_short = 0.0;   // see MatchArgs::strip_span_long
  double beam_rmax = 0.0;
  bool has_search = false;

  DeviceBuffer ws_match, ws_poses, record, stats, outer;
  DeviceBuffer tmp_scores, tmp_poses, tmp_noise;
  // Pipelined pose batches (pipelined_pose_batch): the uploads of a large batch from host memory
  // run on their own stream, piece by piece, under the scoring of the piece before
  hipStream_t up_stream = nullptr, down_stream = nullptr;
  hipEvent_t pipe_up[NDT2D_PIPELINE_PIECES] = {}, pipe_scored[NDT2D_PIPELINE_PIECES] = {}, pipe_idle = nullptr;
  DeviceBuffer piece_stats;   // [pieces][8] moment sums
  int pipeline_pieces = 0;    // 0: default (ndt2d_set_pipeline_pieces)
  int last_pieces = 1;        // pieces of the last host pose batch (ndt2d_last_pipeline_pieces)
  DeviceBuffer near_list;   // ndt2d_match_near_best: {count, indices}
  // LaserScan conversion: ranges (floats), points, {n, rmax | n, use, rmax}
  DeviceBuffer scan_ranges, scan_points, scan_info;
  size_t n_scan_points = 0;

  // HIP events around the dominant kernel of each launch: a ring, so that a caller
  // can queue launches back to back and read their durations afterwards
  hipEvent_t ring0[NDT2D_TIMING_HISTORY] = {}, ring1[NDT2D_TIMING_HISTORY] = {};
  uint64_t n_timed_launches = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // the current launch's pair
  bool timing = true;   // record the event pairs (ndt2d_set_timing)
  bool timed = false;
  int last_kernels = 0;
  const char * last_variant = "";
  int force_variant = ndt2d::kVariantAuto;
  bool batched_only = false;   // "batched": small pose batches stay on the batched kernels
  int eigen_form = 0;          // ndt2d_set_eigenvalue_form (ndt2d_eigen2.h): 0 Eigen's EigenSolver, 1 closed form

  bool match_pending = false;
  uint64_t match_launches = 0, match_fetches = 0;   // searches launched / fetched so far (ndt2d_match_status)
  // a few-pose launch whose results have not been collected (ndt2d_score_poses_beams_launch)
  bool few_pending = false;
  unsigned long long few_seq = 0;
  size_t few_n_poses = 0;
  bool few_stats = false;
  // the moment sums of a sharded particle launch on their way to the host (ndt2d_pose_sums_launch)
  bool sums_pending = false;
  unsigned long long sums_seq = 0;
  uint64_t sums_pos = 0;
  uint64_t last_candidates = 0;
};

namespace ndt2d_device
{

inline int fail(ndt2d_context * h, int code, const std::string & msg)
{
  if (h != nullptr) h->err = msg;
  return code;
}

#ifdef NDT2D_TEST_HOOKS
// Test builds only (libndt2d_hip_hooks.so): the k-th search launch / particle launch from now on
// fails with NDT2D_ERR_HIP (ndt2d_test_fail_launch(k); 0: none) -- how tests/test_gpu_multi_failure.py
// makes ONE device of a multi-device call fail while the others are in flight.
inline std::atomic<int> g_test_fail_launch{0};
inline bool test_launch_fails()
{
  int v = g_test_fail_launch.load();
  while (v > 0)
  {
    if (g_test_fail_launch.compare_exchange_weak(v, v - 1)) return v == 1;
  }
  return false;
}
#define NDT2D_TEST_MAYBE_FAIL(h, what) do { if (test_launch_fails()) return fail(h, NDT2D_ERR_HIP, what ": failure injected by the test hook"); } while (0)
#else
#define NDT2D_TEST_MAYBE_FAIL(h, what) do {} while (0)
#endif

// ndt2d_guard.h: where the text of an exception caught at the C boundary goes
inline void guard_note(ndt2d_context * h, const char * what) noexcept
{
  if (h == nullptr) return;
  try
  {
    h->err = what;
  }
  catch (...)
  {
  }
}
inline void guard_note(std::nullptr_t, const char *) noexcept {}

inline int fail_hip(ndt2d_context * h, hipError_t e, const char * what)
{
  std::string msg = std::string(what) + ": " + hipGetErrorString(e);
  (void)hipGetLastError();  // clear sticky state
  return fail(h, NDT2D_ERR_HIP, msg);
}

#define NDT2D_HIP(h, call)                                 \
  do                                                       \
  {                                                        \
    hipError_t e__ = (call);                               \
    if (e__ != hipSuccess) return fail_hip(h, e__, #call); \
  } while (0)

// hipStreamSynchronize, noting how far the stream has come (see ndt2d_context::reached)
#define NDT2D_SYNC(h)                                          \
  do {                                                         \
    const uint64_t q_ = (h)->queued;                           \
    NDT2D_HIP(h, hipStreamSynchronize((h)->stream));           \
    if ((h)->reached < q_) (h)->reached = q_;                  \
  } while (0)

inline int ensure(ndt2d_context * h, DeviceBuffer & b, size_t doubles)
{
  if (doubles <= b.cap && b.ptr != nullptr) return NDT2D_OK;
  if (b.ptr != nullptr)
  {
    NDT2D_SYNC(h);
    NDT2D_HIP(h, hipFree(b.ptr));
    b.ptr = nullptr;
    b.cap = 0;
  }
  // (an eighth of headroom: the mapper's grid follows the scan poses and grows by a row or
  // a column of cells now and then -- not a free + malloc + stream synchronisation each time)
  size_t cap = doubles < 64 ? 64 : doubles + doubles / 8;
  NDT2D_HIP(h, hipMalloc(reinterpret_cast<void **>(&b.ptr), cap * sizeof(double)));
  b.cap = cap;
  return NDT2D_OK;
}

// Wait until nothing queued reads `st` any more.  After a sequence of synchronous calls the
// stream is already known to be past the buffer's mark (the call that used it ended with a result
// flag); only a caller that queues launch upon launch without fetching waits here.
inline int stage_wait(ndt2d_context * h, PinnedStage & st)
{
  if (st.pending)
  {
    // (nobody has fetched a result since the mark -- back-to-back addScans, say: the stream is
    // asked.  A word the reader raises in host memory when it has read the buffer was tried: it
    // costs the install kernel 1.3 us in every mapper cycle to save 8 us in a sequence no node
    // produces; hipStreamQuery is slower than the synchronisation.)
    if (h->reached < st.needed) NDT2D_SYNC(h);
    st.pending = false;
  }
  return NDT2D_OK;
}

// Make `st` ready to take `doubles` values: wait for the previous copy out of it.
inline int stage_acquire(ndt2d_context * h, PinnedStage & st, size_t doubles)
{
  const int wrc = stage_wait(h, st);
  if (wrc != NDT2D_OK) return wrc;
  if (doubles > st.cap || st.ptr == nullptr)
  {
    if (st.ptr != nullptr) NDT2D_HIP(h, hipHostFree(st.ptr));
    st.ptr = nullptr;
    st.cap = 0;
    const size_t cap = doubles < 4096 ? 4096 : doubles;
    NDT2D_HIP(h, hipHostMalloc(reinterpret_cast<void **>(&st.ptr), cap * sizeof(double), hipHostMallocDefault));
    st.cap = cap;
    st.dev = nullptr;
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&st.dev), st.ptr, 0) != hipSuccess)
    {
      (void)hipGetLastError();
      st.dev = nullptr;
    }
  }
  return NDT2D_OK;
}

// The copy out of a staging buffer, and the mark that tells when the buffer may be written
// again: a POSITION in the in-order stream, not an event.  A recorded event holds the stream
// up for ~5 us in front of whatever is queued next (experiments/kernel_gaps.py; in the mapper's
// cycle 5.8 us between the install kernel and the scoreScan behind it,
// experiments/r03_cycle.sh), and the question it answers is already answered: every
// synchronous call ends with a result flag (or a stream synchronisation) seen by the host,
// which proves everything queued before that kernel done (ndt2d_context::reached).
inline int stage_copy(ndt2d_context * h, PinnedStage & st, double * dst, size_t doubles)
{
  NDT2D_HIP(h, hipMemcpyAsync(dst, st.ptr, doubles * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return NDT2D_OK;
}

inline int stage_mark(ndt2d_context * h, PinnedStage & st)
{
  st.needed = ++h->queued;
  st.pending = true;
  return NDT2D_OK;
}

inline int stage_submit(ndt2d_context * h, PinnedStage & st, double * dst, size_t doubles)
{
  const int rc = stage_copy(h, st, dst, doubles);
  return rc != NDT2D_OK ? rc : stage_mark(h, st);
}

// max |beam|: defined once (ndt2d_context_search.hip), the pose scoring with new beams needs it too
__attribute__((visibility("hidden"))) double beam_reach(const double * beams_xy, size_t n_beams);

constexpr int kScoreFlagSlot = 24;
constexpr int kScoreSlot = 32;                                             // scores / weights of a small batch
constexpr int kPfOutSlot = kScoreSlot + static_cast<int>(ndt2d::kFewPosesMax);   // its statistics
constexpr int kHostResDoubles = kPfOutSlot + 32;

inline int ensure_host_res(ndt2d_context * h)
{
  if (h->host_res != nullptr) return NDT2D_OK;
  void * p = nullptr;
  NDT2D_HIP(h, hipHostMalloc(&p, kHostResDoubles * sizeof(double),
                             hipHostMallocCoherent | hipHostMallocMapped));
  std::memset(p, 0, kHostResDoubles * sizeof(double));
  void * d = nullptr;
  hipError_t e = hipHostGetDevicePointer(&d, p, 0);
  if (e != hipSuccess)
  {
    (void)hipHostFree(p);
    return fail_hip(h, e, "hipHostGetDevicePointer");
  }
  void * counter = nullptr;
  const size_t done_bytes = (static_cast<size_t>(ndt2d::kFewPosesMax) + 8) * sizeof(unsigned long long);
  e = hipMalloc(&counter, done_bytes);
  if (e != hipSuccess)
  {
    (void)hipHostFree(p);
    return fail_hip(h, e, "hipMalloc");
  }
  e = hipMemsetAsync(counter, 0, done_bytes, h->stream);
  if (e != hipSuccess)
  {
    (void)hipHostFree(p);
    (void)hipFree(counter);
    return fail_hip(h, e, "hipMemsetAsync");
  }
  h->host_res = static_cast<double *>(p);
  h->host_res_dev = static_cast<double *>(d);
  h->done_words = static_cast<unsigned long long *>(counter);
  return NDT2D_OK;
}

// Wait until the kernel that was given `seq` has published its results at `slot`:
// spin on the flag for a while (the GPU writes it over PCIe into coherent host memory;
// ~4 us sooner than a stream synchronisation returns), then fall back to the stream.
inline int wait_host_flag(ndt2d_context * h, int slot, unsigned long long seq, uint64_t position)
{
  volatile unsigned long long * flag =
    reinterpret_cast<volatile unsigned long long *>(h->host_res + slot);
  for (int outer = 0; outer < 64; ++outer)
  {
    for (int i = 0; i < 2048; ++i)
    {
      const unsigned long long seen = *flag;
      if (seen == seq)
      {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (h->reached < position) h->reached = position;   // the stream is in order
        return NDT2D_OK;
      }
      if (seen == (seq | ndt2d::kHostFlagGaveUp))
      {
        // the launch's last block waited in vain for another block's result (its bounded poll):
        // this call has no result; the kernel ended normally and the context stays usable
        if (h->reached < position) h->reached = position;
        return fail(h, NDT2D_ERR_HIP, "the kernel gave up waiting for one of its blocks' results (bounded poll)");
      }
      __builtin_ia32_pause();
    }
    // a failed launch / faulted kernel never raises the flag: ask the stream now and then
    const hipError_t q = hipStreamQuery(h->stream);
    if (q != hipErrorNotReady && q != hipSuccess) return fail_hip(h, q, "hipStreamQuery");
  }
  NDT2D_SYNC(h);
  if (*flag == (seq | ndt2d::kHostFlagGaveUp))
  {
    return fail(h, NDT2D_ERR_HIP, "the kernel gave up waiting for one of its blocks' results (bounded poll)");
  }
  if (*flag != seq) return fail(h, NDT2D_ERR_HIP, "result flag was not raised");
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  if (h->reached < position) h->reached = position;
  return NDT2D_OK;
}

// slots of the host-coherent block the sharded particle path uses (behind the few-pose path's
// statistics): a device's eight moment sums, their flag, and its updateStatistics result
constexpr int kPoseSumsSlot = kPfOutSlot + 8;
constexpr int kPoseSumsFlagSlot = kPoseSumsSlot + ndt2d::kPoseSumsFlagOffset;
constexpr int kPfShardOutSlot = kPfOutSlot + 24;
static_assert(kPfShardOutSlot + 8 <= kHostResDoubles, "host block too small");

// Take the next pair of timing events (created on first use) as h->ev0 / h->ev1.
inline int next_timing_slot(ndt2d_context * h)
{
  const size_t slot = static_cast<size_t>(h->n_timed_launches % NDT2D_TIMING_HISTORY);
  if (h->ring0[slot] == nullptr) NDT2D_HIP(h, hipEventCreate(&h->ring0[slot]));
  if (h->ring1[slot] == nullptr) NDT2D_HIP(h, hipEventCreate(&h->ring1[slot]));
  h->ev0 = h->ring0[slot];
  h->ev1 = h->ring1[slot];
  ++h->n_timed_launches;
  return NDT2D_OK;
}

// The address a kernel can use for host memory allocated with ndt2d_host_alloc
// (pinned, mapped); nullptr for ordinary (pageable) host memory.
template <class T>
inline T * device_view(T * host_ptr)
{
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, host_ptr) != hipSuccess)
  {
    (void)hipGetLastError();   // pageable memory: "invalid value", not an error here
    return nullptr;
  }
  if (attr.type != hipMemoryTypeHost || attr.devicePointer == nullptr) return nullptr;
  return static_cast<T *>(attr.devicePointer);
}

inline bool is_pow2(double v)
{
  if (!(v > 0.0) || !std::isfinite(v)) return false;
  int e = 0;
  return std::frexp(v, &e) == 0.5 && std::fpclassify(v) == FP_NORMAL &&
         std::fpclassify(1.0 / v) == FP_NORMAL;
}

}  // namespace ndt2d_device

#pragma GCC visibility pop

#endif  // NDT2D_CONTEXT_H_
