// The sharded calls of a multi-device matcher (ndt2d_matcher_create_multi): matchScan's search and
// ParticleFilter::measure dealt to all devices, one thread per device (ndt2d_workers.h), their
// results exchanged through the host or through RCCL (ndt2d_exchange.h).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host/ndt2d_matcher_state.h"

// (nothing of this unit belongs to the library's dynamic symbol table)
#pragma GCC visibility push(hidden)
namespace ndt2d
{
namespace host
{

// ---------------------------------------------------------------------------
// Multi-device matcher (ndt2d_matcher_create_multi): the sharded calls
// ---------------------------------------------------------------------------

constexpr size_t kRec = NDT2D_MATCH_RECORD_DOUBLES;
constexpr size_t kStats = NDT2D_POSE_STATS_DOUBLES;

// Layout of m->pinned (doubles; n = number of devices):
//   [r n 12 .. (r + 1) n 12)  initial image of device r's record table: zero, its own row {0, -1, 0 ...}
//   zeros [n 12]              initial image of a moment table
//   rows  [n 12]              the table read back from the first device / the rows the host combines
//   sum   [8]                 the summed moments on their way to the devices (host exchange)
size_t pinned_init_off(size_t n, size_t r) { return r * n * kRec; }
size_t pinned_zero_off(size_t n) { return n * n * kRec; }
size_t pinned_rows_off(size_t n) { return n * n * kRec + n * kRec; }
size_t pinned_sum_off(size_t n) { return n * n * kRec + 2 * n * kRec; }
size_t pinned_doubles(size_t n) { return pinned_sum_off(n) + kStats; }

std::string dev_msg_at(ndt2d_matcher * m, size_t r, const char * what)
{
  return std::string(what) + " (device " + std::to_string(m->device_ids[r]) + ", rank " + std::to_string(r) +
         "): " + ndt2d_last_error(m->devs[r]);
}

int dev_fail_at(ndt2d_matcher * m, size_t r, int code, const char * what)
{
  return mfail(m, code, dev_msg_at(m, r, what));
}

// The exchange buffers every sharded call needs: made on the first one.
int ensure_multi(ndt2d_matcher * m)
{
  const size_t n = m->devs.size();
  if (m->pinned == nullptr)
  {
    void * p = nullptr;
    const int rc = ndt2d_host_alloc(m->dev, pinned_doubles(n) * sizeof(double), &p);
    if (rc != NDT2D_OK) return dev_fail_at(m, 0, rc, "ndt2d_host_alloc");
    m->pinned = static_cast<double *>(p);
    std::memset(m->pinned, 0, pinned_doubles(n) * sizeof(double));
    for (size_t r = 0; r < n; ++r) m->pinned[pinned_init_off(n, r) + r * kRec + 1] = -1.0;   // "no candidate"
  }
  for (size_t r = 0; r < n; ++r)
  {
    MatcherShard & sh = m->shards[r];
    if (sh.d_table == nullptr)
    {
      void * d = nullptr;
      int rc = ndt2d_device_alloc(m->devs[r], n * kRec * sizeof(double), &d);
      if (rc != NDT2D_OK) return dev_fail_at(m, r, rc, "ndt2d_device_alloc");
      sh.d_table = static_cast<double *>(d);
      rc = ndt2d_device_alloc(m->devs[r], 2 * kStats * sizeof(double), &d);
      if (rc != NDT2D_OK) return dev_fail_at(m, r, rc, "ndt2d_device_alloc");
      sh.d_sum = static_cast<double *>(d);
    }
  }
  return NDT2D_OK;
}

// Which exchange this call takes (ndt2d_matcher_set_exchange).
int pick_exchange(ndt2d_matcher * m, bool * rccl)
{
  *rccl = false;
  if (m->exchange_mode == 1) return NDT2D_OK;
  if (!m->exchange_tried)
  {
    m->exchange_tried = true;
    std::string why;
    const int rc = ndt2d::exchange_create(&m->exchange, m->device_ids.data(), static_cast<int>(m->device_ids.size()), &why);
    if (rc != NDT2D_OK)
    {
      m->exchange = nullptr;
      m->exchange_note = why;
    }
  }
  if (m->exchange == nullptr)
  {
    if (m->exchange_mode == 2) return mfail(m, NDT2D_ERR_HIP, "exchange \"rccl\" is not available: " + m->exchange_note);
    return NDT2D_OK;   // "auto": the host exchange
  }
  *rccl = true;
  return NDT2D_OK;
}

bool multi_search_wanted(const ndt2d_matcher * m, size_t n_th, size_t n_lin, size_t use)
{
  // (a one-device matcher told to use "rccl" takes the dealt path with one rank: the collective
  // code can then be exercised on a single-GPU box)
  return (m->devs.size() > 1 || m->exchange_mode == 2) && n_th >= 2 &&
         static_cast<double>(n_th) * static_cast<double>(n_lin) * static_cast<double>(n_lin) * static_cast<double>(use) >=
           m->multi_min_units;
}

bool multi_poses_wanted(const ndt2d_matcher * m, size_t n_poses, size_t use)
{
  return (m->devs.size() > 1 || m->exchange_mode == 2) && n_poses >= m->devs.size() &&
         static_cast<double>(n_poses) * static_cast<double>(use) >= m->multi_min_pose_units;
}

void note_variant(ndt2d_matcher * m, bool multi, bool rccl)
{
  m->last_multi = multi;
  m->variant.clear();
  if (multi)
  {
    m->variant = "multi[" + std::to_string(m->devs.size()) + "]/" + (rccl ? "rccl" : "host") + "/";
  }
  m->variant += ndt2d_last_variant(m->dev);
}

// The reference's first-wins rule over the devices' records (src/scan_matcher_ndt.cpp:128, strict
// `<` in visiting order): the lower score, and between equal scores the lower flat index -- the
// candidate the reference's loops visit first; accumulators summed in device order.
// rows[n][12], used[r] = device r searched; out[12].
void combine_records(const double * rows, const std::vector<size_t> & count, double * out)
{
  out[0] = 0.0;
  out[1] = -1.0;
  for (size_t k = 2; k < kRec; ++k) out[k] = 0.0;
  bool first = true;
  for (size_t r = 0; r < count.size(); ++r)
  {
    if (count[r] == 0) continue;
    const double * rec = rows + r * kRec;
    if (rec[1] >= 0.0 && rec[0] < 0.0)
    {
      // (an index ending in .5 is a winner marked "another candidate within the near-tie tolerance": the
      // mark stays with the winner, and two devices' winners that close mark it as well)
      const bool near = out[1] >= 0.0 && std::fabs(rec[0] - out[0]) <=
                                           std::max(std::fabs(rec[0]), std::fabs(out[0])) * NDT2D_NEAR_TIE_REL;
      if (out[1] < 0.0 || rec[0] < out[0] || (rec[0] == out[0] && std::floor(rec[1]) < std::floor(out[1])))
      {
        out[0] = rec[0];
        out[1] = rec[1];
      }
      if (near) out[1] = std::floor(out[1]) + 0.5;
    }
    // (the first device's sums are taken as they are: one device gives the single-device bits)
    for (size_t k = 2; k < kRec; ++k) out[k] = first ? rec[k] : out[k] + rec[k];
    first = false;
  }
}

// What one device's thread reports of its part of a dealt call (the message is made by the
// calling thread afterwards: ndt2d_matcher::err is not the threads' to write).
struct RankStatus
{
  int rc = NDT2D_OK;
  const char * what = "";
};

double elapsed_us(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// A dealt call is given up: nothing of it may stay in flight once the caller has the error -- copies
// out of / into the caller's buffers, searches launched but not fetched.  Every device is waited out.
void drain_devices(ndt2d_matcher * m)
{
  for (ndt2d_handle h : m->devs)
  {
    uint64_t launched = 0, fetched = 0;
    if (ndt2d_match_status(h, &launched, &fetched) == NDT2D_OK && launched > fetched)
    {
      ndt2d_match_result res;
      (void)ndt2d_match_fetch(h, &res);
    }
    (void)ndt2d_synchronize(h);
  }
}

// msg is made by the caller, before the devices are touched again.
int give_up_dealt(ndt2d_matcher * m, int code, const std::string & msg)
{
  mfail(m, code, msg);
  drain_devices(m);
  return code;
}

int first_failure(ndt2d_matcher * m, const std::vector<RankStatus> & st)
{
  for (size_t r = 0; r < st.size(); ++r)
  {
    if (st[r].rc != NDT2D_OK) return give_up_dealt(m, st[r].rc, dev_msg_at(m, r, st[r].what));
  }
  return NDT2D_OK;
}

// matchScan's search dealt to all devices.  The first device has been prepared by the caller
// (beams + tables); m->beams holds the subsampled beams unless `beams_everywhere` (every device
// converted the LaserScan itself).  all_scores (host, optional): the whole lattice's scores.
// Every device's tables, beams and launch go out on its own thread (ndt2d_workers.h).
int multi_match(ndt2d_matcher * m, const double * scan_pose_xyt, size_t n_th, size_t n_lin, size_t use,
                bool beams_everywhere, double * all_scores, double * record_out)
{
  const size_t n = m->devs.size();
  const auto t_start = std::chrono::steady_clock::now();
  int rc = ensure_multi(m);
  if (rc != NDT2D_OK) return rc;
  bool rccl = false;
  if ((rc = pick_exchange(m, &rccl)) != NDT2D_OK) return rc;
  const size_t per_th = n_lin * n_lin;
  std::vector<size_t> count(n, 0);
  for (size_t r = 0; r < n; ++r) count[r] = r < n_th ? (n_th - r + n - 1) / n : 0;
  if (all_scores != nullptr)
  {
    for (size_t r = 0; r < n; ++r)
    {
      MatcherShard & sh = m->shards[r];
      const size_t want = count[r] * per_th;
      if (want > sh.scores_cap)
      {
        if (sh.d_scores != nullptr) ndt2d_device_free(m->devs[r], sh.d_scores);
        sh.d_scores = nullptr;
        sh.scores_cap = 0;
        void * d = nullptr;
        rc = ndt2d_device_alloc(m->devs[r], want * sizeof(double), &d);
        if (rc != NDT2D_OK) return dev_fail_at(m, r, rc, "ndt2d_device_alloc");
        sh.d_scores = static_cast<double *>(d);
        sh.scores_cap = want;
      }
    }
  }
  // every device's search goes out before any result is waited for, all of them side by side
  std::vector<RankStatus> st(n);
  m->fanout_us.assign(n, 0.0);
  auto deal = [&](size_t r) {
    RankStatus & s = st[r];
    MatcherShard & sh = m->shards[r];
    if (r > 0)
    {
      s.what = "ndt2d_set_search_beams";
      if (beams_everywhere)
      {
        s.rc = ndt2d_set_search(m->devs[r], scan_pose_xyt[0], scan_pose_xyt[1], m->search.dth.data(),
                                m->search.cos_th.data(), m->search.sin_th.data(), n_th, m->search.dlin.data(), n_lin);
      }
      else
      {
        s.rc = ndt2d_set_search_beams(m->devs[r], m->beams.host.data(), use, scan_pose_xyt[0], scan_pose_xyt[1],
                                      m->search.dth.data(), m->search.cos_th.data(), m->search.sin_th.data(), n_th,
                                      m->search.dlin.data(), n_lin);
      }
      sh.beams_epoch = ~0ull;   // (the device's beams now live in the search's upload)
      if (s.rc != NDT2D_OK) return;
    }
    if (rccl)
    {
      s.what = "ndt2d_copy_to_device_async";
      s.rc = ndt2d_copy_to_device_async(m->devs[r], sh.d_table, m->pinned + pinned_init_off(n, r), n * kRec * sizeof(double));
      if (s.rc != NDT2D_OK) return;
    }
    if (count[r] > 0)
    {
      s.what = "ndt2d_match_launch_strided";
      s.rc = ndt2d_match_launch_strided(m->devs[r], r, n, count[r], all_scores != nullptr ? sh.d_scores : nullptr,
                                        rccl ? sh.d_table + r * kRec : nullptr);
    }
    m->fanout_us[r] = elapsed_us(t_start);
  };
  m->workers->run(deal);
  if ((rc = first_failure(m, st)) != NDT2D_OK) return rc;
  double * rows = m->pinned + pinned_rows_off(n);
  if (rccl)
  {
    // the ONE collective of the search: all-reduce(sum) of the [n, 12] table, every device its own row
    std::vector<double *> tables(n);
    std::vector<void *> streams(n);
    for (size_t r = 0; r < n; ++r)
    {
      tables[r] = m->shards[r].d_table;
      streams[r] = ndt2d_get_stream(m->devs[r]);
    }
    std::string why;
    rc = ndt2d::exchange_all_reduce(m->exchange, tables.data(), n * kRec, streams.data(), &why);
    if (rc != NDT2D_OK) return give_up_dealt(m, rc, why);
    rc = ndt2d_copy_to_host_async(m->dev, rows, m->shards[0].d_table, n * kRec * sizeof(double));
    if (rc == NDT2D_OK) rc = ndt2d_synchronize(m->dev);
    if (rc != NDT2D_OK) return give_up_dealt(m, rc, dev_msg_at(m, 0, "ndt2d_copy_to_host_async"));
  }
  for (size_t r = 0; r < n; ++r)
  {
    if (count[r] == 0) continue;
    // host exchange: the record through the context's host-coherent result block.  (After an
    // all-reduce the flags are up already -- every stream's collective follows its search --
    // and the fetch only settles the context's state.)
    ndt2d_match_result res;
    rc = ndt2d_match_fetch(m->devs[r], &res);
    if (rc != NDT2D_OK) return give_up_dealt(m, rc, dev_msg_at(m, r, "ndt2d_match_fetch"));
    if (!rccl) record_from(res, rows + r * kRec);
  }
  if (all_scores != nullptr)
  {
    // device r holds the scores of the steps r, r + n, ... in that order
    std::vector<double> tmp;
    for (size_t r = 0; r < n; ++r)
    {
      if (count[r] == 0) continue;
      tmp.resize(count[r] * per_th);
      rc = ndt2d_copy_to_host(m->devs[r], tmp.data(), m->shards[r].d_scores, tmp.size() * sizeof(double));
      if (rc != NDT2D_OK) return give_up_dealt(m, rc, dev_msg_at(m, r, "ndt2d_copy_to_host"));
      for (size_t k = 0; k < count[r]; ++k)
      {
        std::memcpy(all_scores + (r + k * n) * per_th, tmp.data() + k * per_th, per_th * sizeof(double));
      }
    }
  }
  combine_records(rows, count, record_out);
  note_variant(m, true, rccl);
  return NDT2D_OK;
}

// The prepared search run: dealt to all devices when it is large enough (multi_match, which
// takes beams_everywhere and scores as it does), else on the first.  record: marked, record_from.
int run_search(ndt2d_matcher * m, const double * scan_pose_xyt, size_t n_th, size_t n_lin, size_t use,
               bool beams_everywhere, double * scores, double * record)
{
  if (multi_search_wanted(m, n_th, n_lin, use))
  {
    return multi_match(m, scan_pose_xyt, n_th, n_lin, use, beams_everywhere, scores, record);
  }
  ndt2d_match_result res;
  const int rc = ndt2d_match(m->dev, 0, n_th, scores, &res);
  if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_match");
  record_from(res, record);
  return NDT2D_OK;
}

// Room for `n_poses` particles and their weights on device r.
int ensure_shard_poses(ndt2d_matcher * m, size_t r, size_t n_poses)
{
  MatcherShard & sh = m->shards[r];
  if (n_poses <= sh.poses_cap) return NDT2D_OK;
  if (sh.d_poses != nullptr) ndt2d_device_free(m->devs[r], sh.d_poses);
  if (sh.d_weights != nullptr) ndt2d_device_free(m->devs[r], sh.d_weights);
  sh.d_poses = sh.d_weights = nullptr;
  sh.poses_cap = 0;
  const size_t cap = n_poses + n_poses / 8;
  void * d = nullptr;
  int rc = ndt2d_device_alloc(m->devs[r], 3 * cap * sizeof(double), &d);
  if (rc != NDT2D_OK) return dev_fail_at(m, r, rc, "ndt2d_device_alloc");
  sh.d_poses = static_cast<double *>(d);
  rc = ndt2d_device_alloc(m->devs[r], cap * sizeof(double), &d);
  if (rc != NDT2D_OK) return dev_fail_at(m, r, rc, "ndt2d_device_alloc");
  sh.d_weights = static_cast<double *>(d);
  sh.poses_cap = cap;
  return NDT2D_OK;
}

// Contiguous share [begin, end) of n items for rank r of `world` (sizes differ by at most one).
void shard_range(size_t n, size_t r, size_t world, size_t * begin, size_t * end)
{
  const size_t base = n / world, rem = n % world;
  *begin = r * base + std::min(r, rem);
  *end = *begin + base + (r < rem ? 1 : 0);
}

// scorePoses / ParticleFilter::measure over all devices: contiguous particle ranges.  The first
// device holds the beams (the caller staged them), m->beams is their host copy.  stats_out ==
// nullptr: scores only.  Otherwise the whole of measure: scores_out receives the normalised
// weights and stats_out NDT2D_PF_RESULT_DOUBLES values as ndt2d_pf_finalize_launch defines them
// ([7] summed over the devices in device order).
//
// Every device's share runs on its own thread from the upload to the weights' way back.  Host
// exchange: the device's eight moment sums arrive in its host-coherent block behind a flag
// (ndt2d_pose_sums_fetch), the threads meet (DeviceWorkers::barrier), each adds the rows in device
// order -- the "total particle weight" of src/particle_filter.cpp:166-174 -- and launches
// updateStatistics with the totals as kernel arguments: no copy and no stream synchronisation
// between the two halves.  RCCL exchange: the shares are dealt the same way, the two
// all-reduces are issued by the calling thread.
int multi_score_poses(ndt2d_matcher * m, const double * poses_xyt, size_t n_poses, size_t use, double * scores_out,
                      double * stats_out)
{
  const size_t n = m->devs.size();
  const auto t_start = std::chrono::steady_clock::now();
  int rc = ensure_multi(m);
  if (rc != NDT2D_OK) return rc;
  bool rccl = false;
  if (stats_out != nullptr && (rc = pick_exchange(m, &rccl)) != NDT2D_OK) return rc;
  std::vector<size_t> begin(n), end(n);
  for (size_t r = 0; r < n; ++r)
  {
    shard_range(n_poses, r, n, &begin[r], &end[r]);
    if ((rc = ensure_shard_poses(m, r, end[r] - begin[r])) != NDT2D_OK) return rc;
  }
  const double * zeros = m->pinned + pinned_zero_off(n);
  double * rows = m->pinned + pinned_rows_off(n);
  std::vector<RankStatus> st(n);
  m->fanout_us.assign(n, 0.0);
  std::atomic<bool> give_up{false};
  // (host exchange: the devices' rows of sums and of results, written by their threads)
  std::vector<double> sums(n * kStats, 0.0), results(n * kStats, 0.0);
  const bool host_measure = stats_out != nullptr && !rccl;

  auto share = [&](size_t r) {
    RankStatus & s = st[r];
    MatcherShard & sh = m->shards[r];
    const size_t nr = end[r] - begin[r];
    auto fail = [&](const char * what, bool sync) {
      s.what = what;
      give_up.store(true, std::memory_order_release);
      if (sync) (void)ndt2d_synchronize(m->devs[r]);   // nothing of this share stays in flight
    };
    if (r > 0 && sh.beams_epoch != m->beams.epoch)
    {
      if ((s.rc = ndt2d_set_beams(m->devs[r], m->beams.host.data(), use)) != NDT2D_OK) return fail("ndt2d_set_beams", true);
      sh.beams_epoch = m->beams.epoch;
    }
    s.rc = ndt2d_copy_to_device_async(m->devs[r], sh.d_poses, poses_xyt + 3 * begin[r], 3 * nr * sizeof(double));
    if (s.rc == NDT2D_OK && rccl)
    {
      s.rc = ndt2d_copy_to_device_async(m->devs[r], sh.d_table, zeros, n * kStats * sizeof(double));
    }
    if (s.rc != NDT2D_OK) return fail("ndt2d_copy_to_device_async", true);
    if (!host_measure)
    {
      // scores only, or the first half of the RCCL form (the moment sums into the device's row)
      double * d_stats = stats_out == nullptr ? nullptr : sh.d_table + r * kStats;
      s.rc = ndt2d_score_poses_launch(m->devs[r], sh.d_poses, nr, sh.d_weights, d_stats);
      m->fanout_us[r] = elapsed_us(t_start);
      if (s.rc != NDT2D_OK) return fail("ndt2d_score_poses_launch", true);
      if (stats_out == nullptr)
      {
        s.rc = ndt2d_copy_to_host_async(m->devs[r], scores_out + begin[r], sh.d_weights, nr * sizeof(double));
        if (s.rc == NDT2D_OK) s.rc = ndt2d_synchronize(m->devs[r]);
        if (s.rc != NDT2D_OK) return fail("ndt2d_copy_to_host_async", true);
      }
      return;
    }
    s.rc = ndt2d_pose_sums_launch(m->devs[r], sh.d_poses, nr, sh.d_weights);
    m->fanout_us[r] = elapsed_us(t_start);
    if (s.rc != NDT2D_OK) return fail("ndt2d_pose_sums_launch", true);
    if ((s.rc = ndt2d_pose_sums_fetch(m->devs[r], sums.data() + r * kStats)) != NDT2D_OK) return fail("ndt2d_pose_sums_fetch", true);
    if (!m->workers->barrier(give_up))
    {
      // another device's share failed (its status says how) or never came: this one is abandoned
      if (!give_up.load()) { s.rc = NDT2D_ERR_HIP; fail("the devices' moment sums did not meet", false); }
      (void)ndt2d_synchronize(m->devs[r]);
      return;
    }
    // the rows summed in device order: the same bits on every thread
    double totals[kStats];
    for (size_t k = 0; k < kStats; ++k)
    {
      double acc = sums[k];
      for (size_t q = 1; q < n; ++q) acc += sums[q * kStats + k];
      totals[k] = acc;
    }
    // updateStatistics with the total sums: normalised weights, the mean and covariance (the same
    // on all devices), and the device's part of the theta variance (:213-217)
    s.rc = ndt2d_pf_finalize_totals_launch(m->devs[r], sh.d_poses, nr, sh.d_weights, totals);
    if (s.rc != NDT2D_OK) return fail("ndt2d_pf_finalize_totals_launch", true);
    s.rc = ndt2d_copy_to_host_async(m->devs[r], scores_out + begin[r], sh.d_weights, nr * sizeof(double));
    if (s.rc == NDT2D_OK) s.rc = ndt2d_synchronize(m->devs[r]);
    if (s.rc != NDT2D_OK) return fail("ndt2d_copy_to_host_async", true);
    if ((s.rc = ndt2d_pf_result_read(m->devs[r], results.data() + r * kStats)) != NDT2D_OK) return fail("ndt2d_pf_result_read", false);
  };
  m->workers->run(share);
  if ((rc = first_failure(m, st)) != NDT2D_OK) return rc;
  if (host_measure)
  {
    for (size_t k = 0; k < NDT2D_PF_RESULT_DOUBLES; ++k) stats_out[k] = results[k];
    for (size_t r = 1; r < n; ++r) stats_out[7] += results[r * kStats + 7];
    note_variant(m, true, false);
    return NDT2D_OK;
  }
  if (stats_out == nullptr)
  {
    note_variant(m, true, false);
    return NDT2D_OK;
  }

  // RCCL exchange.  On any failure from here on every device is waited out before the error returns.
  std::vector<double *> tables(n);
  std::vector<void *> streams(n);
  for (size_t r = 0; r < n; ++r)
  {
    tables[r] = m->shards[r].d_table;
    streams[r] = ndt2d_get_stream(m->devs[r]);
  }
  std::string why;
  // the "total particle weight" all-reduce (src/particle_filter.cpp:166-174) with the other
  // seven moment sums: [n, 8], every device its own row -- the ONE collective of the call
  // (until round 6 the devices' theta-variance parts went through a second one)
  rc = ndt2d::exchange_all_reduce(m->exchange, tables.data(), n * kStats, streams.data(), &why);
  if (rc != NDT2D_OK) return give_up_dealt(m, rc, why);
  // Behind it every device goes on by itself, on its own thread: the rows summed in device order
  // (the same bits everywhere), updateStatistics with them -- normalised weights, mean and
  // covariance, and the device's OWN part of the theta variance (:213-217) -- then the weights and
  // the eight results travel home together; the parts are added below, in device order.
  for (RankStatus & s : st) s = RankStatus();
  std::vector<std::string> whys(n);
  auto finish = [&](size_t r) {
    RankStatus & s = st[r];
    MatcherShard & sh = m->shards[r];
    const size_t nr = end[r] - begin[r];
    s.what = "sum_rows_launch";
    s.rc = ndt2d::sum_rows_launch(m->device_ids[r], tables[r], static_cast<int>(n), static_cast<int>(kStats), sh.d_sum,
                                  streams[r], &whys[r]);
    if (s.rc == NDT2D_OK)
    {
      s.what = "ndt2d_pf_finalize_launch";
      s.rc = ndt2d_pf_finalize_launch(m->devs[r], sh.d_poses, nr, sh.d_weights, sh.d_sum, sh.d_sum + kStats);
    }
    if (s.rc == NDT2D_OK)
    {
      s.what = "ndt2d_copy_to_host_async";
      s.rc = ndt2d_copy_to_host_async(m->devs[r], scores_out + begin[r], sh.d_weights, nr * sizeof(double));
    }
    if (s.rc == NDT2D_OK)
    {
      s.rc = ndt2d_copy_to_host_async(m->devs[r], rows + r * kStats, sh.d_sum + kStats, kStats * sizeof(double));
    }
    const int src = ndt2d_synchronize(m->devs[r]);   // (whatever happened: nothing of this device stays in flight)
    if (s.rc == NDT2D_OK) s.rc = src;
  };
  m->workers->run(finish);
  if ((rc = first_failure(m, st)) != NDT2D_OK) return rc;
  for (size_t k = 0; k < NDT2D_PF_RESULT_DOUBLES; ++k) stats_out[k] = rows[k];
  for (size_t r = 1; r < n; ++r) stats_out[7] += rows[r * kStats + 7];
  note_variant(m, true, true);
  return NDT2D_OK;
}

}  // namespace host
}  // namespace ndt2d
#pragma GCC visibility pop
