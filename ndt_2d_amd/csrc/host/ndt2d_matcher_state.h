// What the matcher's translation units share (ndt2d_host.cpp, host/ndt2d_multi.cpp, host/ndt2d_batched.cpp):
// struct ndt2d_matcher -- the reference's ScanMatcherNDT object restated over the device layer -- with
// the owners of its parts (the beams on the device, the prepared search, the search launched ahead,
// the NDT in place), the error helpers, and the functions that cross those units.  Nothing here is
// part of the C-ABI: everything is hidden from the library's dynamic symbol table.
#ifndef NDT2D_MATCHER_STATE_H_
#define NDT2D_MATCHER_STATE_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host/ndt2d_host_ndt.h"
#include "ndt2d_exchange.h"
#include "ndt2d_hip.h"
#include "ndt2d_workers.h"

// What one device of a multi-device matcher keeps for the sharded calls (device memory of
// ITS GPU, sized on demand).
struct MatcherShard
{
  double * d_table = nullptr;     // [n_dev][12] record / [n_dev][8] moment table of the exchange
  double * d_sum = nullptr;       // 8 moment sums (all devices) | 8 statistics of this device
  double * d_scores = nullptr;    // per-candidate scores of this device's theta steps (optional)
  size_t scores_cap = 0;
  double * d_poses = nullptr;     // this device's particle range
  double * d_weights = nullptr;
  size_t poses_cap = 0;
  uint64_t beams_epoch = ~0ull;   // ndt2d_matcher::beams.epoch of the beams ndt2d_set_beams put there
};

#pragma GCC visibility push(hidden)

namespace ndt2d
{
namespace host
{

// Two scans' subsampled beams, bit for bit the same (and not none).
inline bool same_beams(const std::vector<double> & a, const std::vector<double> & b)
{
  return !a.empty() && a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

}  // namespace host
}  // namespace ndt2d

// (the public header names this type, so it keeps the default visibility -- and says so about its
// hidden members' types; nothing outside the library sees more of it than the name)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wattributes"
struct ndt2d_matcher
{
  ndt2d_handle dev = nullptr;            // == devs[0]: every single-pose and small call runs here
  std::vector<ndt2d_handle> devs;        // one context per entry of device_ids
  std::vector<int> device_ids;
  std::vector<MatcherShard> shards;
  int exchange_mode = 0;                 // 0 auto, 1 host, 2 rccl (ndt2d_matcher_set_exchange)
  ndt2d::Exchange * exchange = nullptr;  // RCCL communicators, made when first needed
  bool exchange_tried = false;
  std::string exchange_note;             // why "auto" did not take RCCL
  // Work below these stays on the first device: candidates x beams of a search (~0.3 ms of one
  // GPU) and particles x beams of a batch (~0.2 ms; BASELINE configs[4], 7.2e8, is above it).
  // Dealing costs the call ~25 us over its slowest share (profiles/r05_multi_device_summary.json).
  double multi_min_units = 1.0e9;
  double multi_min_pose_units = 2.0e8;
  std::unique_ptr<ndt2d::DeviceWorkers> workers;   // one thread per device beyond the first
  std::vector<double> fanout_us;         // last dealt call: when each device's launch was queued
  double * pinned = nullptr;             // host block of the exchanges (layout: multi_pinned_*)
  std::string variant;                   // ndt2d_matcher_last_variant
  bool last_multi = false;
  std::string err;
  // the six declared parameters, reference src/scan_matcher_ndt.cpp:37-44
  double resolution = 0.25;
  double angular_res = 0.0025, angular_size = 0.1;
  double linear_res = 0.005, linear_size = 0.05;
  size_t laser_max_beams = 100;
  double range_max = 0.0;
  int build_mode = 0;             // 0 auto, 1 host, 2 device, 3 fused
  std::vector<ndt2d_scanstore *> stores;   // resident scans, one store per device (made by the first store_scan)
  ndt2d_closure * closure = nullptr;       // batched loop-closure match on the first device (made by the first match_candidates)
  std::vector<double> closure_records;     // its records, [K][NDT2D_MATCH_RECORD_DOUBLES]
  ndt2d_starts * starts = nullptr;         // batched match from K start poses on the first device (made by the first match_starts)
  std::vector<double> starts_records;      // its records, [K][NDT2D_MATCH_RECORD_DOUBLES]
  ndt2d_wide * wide = nullptr;             // wide search on the first device (made by the first match_wide)
  uint64_t wide_installs = ~0ull;          // ndt.installs() at its last call: the same, and its bound image is of this NDT
  ndt2d_scans * scans = nullptr;           // batched scan tracking on the first device (made by the first match_scans)
  std::vector<double> scans_records;       // its records, [K][NDT2D_MATCH_RECORD_DOUBLES]
  ndt2d_refine * refine = nullptr;         // Newton registration on the first device (made by the first refine_scans)
  std::vector<double> refine_records;      // its records, [K][NDT2D_REFINE_RECORD_DOUBLES]
  uint32_t refine_cells = 1;               // the neighbourhood of the later refine_scans: 1 or 9 (set_refine_neighbourhood)
  ndt2d_verify * verify = nullptr;         // match verification on the first device (made by the first verify_scans)
  uint32_t verify_cells = 9;               // the parameters of the later verify_scans (set_verify_*): 1 or 9 cells,
  double verify_gate_inlier = 9.0, verify_gate_pierce = 1.0;   // the gates,
  bool verify_rays = true;                 // the ray walk
  int eigen_form = ndt2d::kEigenFormSchur;   // ndt2d_matcher_set_eigenvalue_form

  // The NDT in place: `ndt_` of the reference (scan_matcher_ndt.hpp:102) -- the grid every device of
  // the matcher holds, how it was built, and the host's copies of it.  Changed by begin_build /
  // built_on_* / drop / give_up / fetched_back only; nothing else in the matcher layer clears a device's grid.
  class NdtInPlace
  {
  public:
    typedef ndt2d::host::HostNdt HostNdt;
    bool have() const { return have_; }
    // it came from the fused build: one pose at a time is scored on the device (fetching the grid
    // back for the host path would cost the cycle more than the build saved)
    bool fused() const { return fused_; }
    const char * last_build() const { return have_ ? build_ : ""; }   // ndt2d_matcher_last_build
    // counts the builds and drops: what was derived from the grid on the devices is stale once it moved
    uint64_t installs() const { return installs_; }
    const HostNdt * built() const { return host_.get(); }             // the host build's own NDT; none after a device build
    // ... or else the copy fetched back from the device, if one was (host_ndt())
    const HostNdt * host_copy() const { return host_ ? host_.get() : fetched_.get(); }

    // A build replaces the NDT in place: there is none until built_on_*.  Returns the storage of the
    // host copy, or what drop() kept, for a host build to fill (a device build lets it go).
    std::unique_ptr<HostNdt> begin_build() { forget(); return std::move(spare_); }
    // ... installed on every device
    void built_on_host(std::unique_ptr<HostNdt> ndt) { host_ = std::move(ndt); have_ = true; build_ = "build/host"; }
    // ... by every device: the host has no copy
    void built_on_device(bool fused) { have_ = true; fused_ = fused; build_ = fused ? "build/fused-small-map" : "build/device"; }
    // `ndt_.reset()`: no NDT on any device (the host copy's storage serves the next build).  The first
    // error of the clears.
    int drop(const std::vector<ndt2d_handle> & devs)
    {
      forget();
      int rc = NDT2D_OK;
      for (ndt2d_handle h : devs)
      {
        const int crc = ndt2d_clear_grid(h);
        if (rc == NDT2D_OK) rc = crc;
      }
      return rc;
    }
    // ... which is what every failure after a device was touched leaves; `code` (whose message was made
    // before the devices are talked to again) is returned
    int give_up(const std::vector<ndt2d_handle> & devs, int code) { (void)drop(devs); return code; }
    // the grid a device built, fetched back once: it belongs to the grid now on the device
    const HostNdt * fetched_back(std::unique_ptr<HostNdt> ndt) { fetched_ = std::move(ndt); return fetched_.get(); }

  private:
    void forget()
    {
      if (host_) spare_ = std::move(host_);
      fetched_.reset();
      have_ = fused_ = false;
      build_ = "";
      ++installs_;
    }
    uint64_t installs_ = 0;
    std::unique_ptr<HostNdt> host_, spare_, fetched_;
    bool have_ = false, fused_ = false;
    const char * build_ = "";
  } ndt;

  // What the first device holds as its beams: a scoring call that arrives with the same points
  // again (the unchanged ParticleFilter::measure calls scorePoints once per particle with one
  // scan, src/particle_filter.cpp:81-87; the mapper calls scoreScan and matchScan on one scan,
  // src/ndt_mapper.cpp:514-515) skips the upload.  The matcher must be the only writer of its
  // context's beams.  Changed by adopt / sent / lost only.
  struct DeviceBeams
  {
    std::vector<double> host;    // host copy of the subsampled beams (empty: a LaserScan the device converted)
    std::vector<double> next;    // the subsampled beams of the call now arriving
    bool on_device = false;      // the first device holds `host`
    uint64_t epoch = 0;          // counts the changes of `host` (MatcherShard::beams_epoch is compared with it)
    bool holds(const std::vector<double> & b) const { return on_device && ndt2d::host::same_beams(host, b); }
    // b becomes the host copy, not yet on the device (b is left with the old one)
    void adopt(std::vector<double> & b) { host.swap(b); ++epoch; on_device = false; }
    void sent() { on_device = true; }    // the device received `host` (an upload, or a launch that carried it)
    void lost() { on_device = false; }   // a call that may have replaced it failed
  } beams;

  // The prepared search: the visited offsets (set by initialize()), the per-theta cos/sin and
  // the beams of the last prepare_search / match_laser_scan / search launched ahead.
  struct PreparedSearch
  {
    std::vector<double> dth, dlin, cos_th, sin_th;
    size_t n_use = 0;     // beams in use (the N of `best / N`, :148)
    bool ready = false;   // the first device holds the tables (and the beams) of it
  } search;

  // The mapper calls scoreScan(scan) and then matchScan(scan, ...) (reference
  // src/ndt_mapper.cpp:514-515, 552-553).  Once that pair has been seen, scoreScan queues the
  // scan's search behind its own kernel before it waits for the score: the search then starts
  // when the scoring kernel ends, not a host round trip later, and the matchScan that follows
  // only collects it.  A call that is not that matchScan waits the search out, discards it, and
  // scoreScan stops doing it until the pair is seen again.  Changed by the *_ahead and
  // note_*_scan functions only (and the switch).
  struct SearchAhead
  {
    bool enabled = true;          // ndt2d_matcher_set_search_ahead
    bool pair_seen = false;       // the last matchScan was of the scan and pose of the scoreScan before it
    bool after_score_scan = false;   // the previous device call was a scoreScan ...
    double score_scan_pose[3] = {0.0, 0.0, 0.0};   // ... from this pose ...
    std::vector<double> scored;   // ... of these subsampled beams
    bool pending = false;         // a search launched by scoreScan has not been collected
    double pose[3] = {0.0, 0.0, 0.0};
    size_t n_th = 0;
    uint64_t launch_id = 0, fetch_id = 0;   // ndt2d_match_status right after that launch
    uint64_t launched = 0, collected = 0;   // ndt2d_matcher_search_ahead_stats
  } ahead;

  std::vector<float> scratch_ranges;   // ranges with their kept infinities made finite (off_grid_ranges)
  // near-tie adjudication (ndt2d_matcher_set_adjudication)
  bool adjudicate = true;
  uint64_t adj_marked = 0, adj_changed = 0, adj_truncated = 0;
  // One pose at a time (scorePoints, scoreScan): scored on the host from the host NDT when the
  // scan is short (ndt2d_matcher_set_single_pose_path).
  bool single_pose_host = true;
  size_t single_pose_max_beams = 256;
};
#pragma GCC diagnostic pop

namespace ndt2d
{
namespace host
{

// ndt2d_guard.h: where the text of an exception caught at the C boundary goes
inline void guard_note(ndt2d_matcher * m, const char * what) noexcept
{
  if (m == nullptr) return;
  try
  {
    m->err = what;
  }
  catch (...)
  {
  }
}
inline void guard_note(std::nullptr_t, const char *) noexcept {}

inline int mfail(ndt2d_matcher * m, int code, const std::string & msg)
{
  if (m != nullptr) m->err = msg;
  return code;
}

inline const char * eigen_form_name(const ndt2d_matcher * m)
{
  return m->eigen_form == ndt2d::kEigenFormClosed ? "closed" : "eigen";
}

inline int dev_fail(ndt2d_matcher * m, int code, const char * what)
{
  return mfail(m, code, std::string(what) + ": " + ndt2d_last_error(m->dev));
}

// A search's result as the record {best_score, best_index or -1, k00,k01,k02,k11,k12,k22, u0,u1,u2, s};
// a winner with another candidate within the near-tie tolerance is marked: index + 0.5.
inline void record_from(const ndt2d_match_result & res, double * rec)
{
  rec[0] = res.best_score;
  rec[1] = res.best_index == NDT2D_NO_INDEX ? -1.0 : static_cast<double>(res.best_index) + (res.near_tie ? 0.5 : 0.0);
  for (int i = 0; i < 10; ++i) rec[2 + i] = res.acc[i];
}

// Is the record's winner marked?
inline bool marked_winner(const double * rec)
{
  const double bi = rec[1];
  return bi >= 0.0 && bi != std::floor(bi);
}

// The record's best index as the C-ABI reports it (a mark is truncated away).
inline uint64_t record_best_index(const double * rec)
{
  return rec[1] < 0.0 ? NDT2D_NO_INDEX : static_cast<uint64_t>(rec[1]);
}

// ---- ndt2d_host.cpp ----

// A search launched ahead that the call now arriving cannot use: waited out and dropped.
void discard_ahead(ndt2d_matcher * m);

// Subsample `points` (src/scan_matcher_ndt.cpp:95-96,110) into the matcher's host copy of the beams
// -- the context's beams are not touched -- as the scan of a search that is not prepared yet:
// search.n_use = the beams in use (returned), search.ready = false.  *held_out: the first device
// holds exactly these beams already.
size_t adopt_scan(ndt2d_matcher * m, const double * points_xy, size_t n_points, bool * held_out = nullptr);

// search.cos_th / sin_th of scan_pose.theta + dth, per theta step (src/scan_matcher_ndt.cpp:106-107)
void fill_rotations(ndt2d_matcher * m, double scan_theta);

// ---- host/ndt2d_multi.cpp ----

int dev_fail_at(ndt2d_matcher * m, size_t r, int code, const char * what);
bool multi_search_wanted(const ndt2d_matcher * m, size_t n_th, size_t n_lin, size_t use);
bool multi_poses_wanted(const ndt2d_matcher * m, size_t n_poses, size_t use);
void note_variant(ndt2d_matcher * m, bool multi, bool rccl);
int run_search(ndt2d_matcher * m, const double * scan_pose_xyt, size_t n_th, size_t n_lin, size_t use,
               bool beams_everywhere, double * scores, double * record);
int multi_score_poses(ndt2d_matcher * m, const double * poses_xyt, size_t n_poses, size_t use, double * scores_out,
                      double * stats_out);

}  // namespace host
}  // namespace ndt2d

#pragma GCC visibility pop

#endif  // NDT2D_MATCHER_STATE_H_
