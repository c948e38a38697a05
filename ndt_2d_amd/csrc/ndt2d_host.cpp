// The matcher of libndt2d_hip.so (include/ndt2d_hip.h, section 2): ndt2d_matcher_*, the reference's
// ScanMatcherNDT object restated over the device layer -- subsampling, search tables, the search
// launched ahead, near-tie settling, the final covariance formula -- and the batched particle path
// (ParticleFilter::measure).  The rest of the host side lies under host/:
//   * ndt2d_host_ndt.h / .cpp   HostNdt, the bit-faithful NDT build of addScans on the host; the
//                               search lattice's offsets; subsampling,
//   * ndt2d_matcher_state.h     struct ndt2d_matcher and what the matcher's units share,
//   * ndt2d_multi.cpp           the calls dealt to all devices of a multi-device matcher,
//   * ndt2d_batched.cpp         match_candidates / match_starts / match_scans,
//   * ndt2d_job_batch.h         the (scan, pose) job list of the batched calls: refusals, batch, way back,
//   * ndt2d_kld.cpp, ndt2d_synth.cpp   the host KLD resampler, the synthetic workload generator.
// Scoring arithmetic on the HOST exists in exactly two places, both by design
// and neither a fallback -- a matcher cannot be created without a GPU: (1) one pose of a scan
// of at most 256 subsampled beams (scorePoints / scoreScan as the unchanged
// ParticleFilter::measure calls them, once per particle: a launch + PCIe round trip per call
// costs 25x the arithmetic) is scored by the calling thread from the host copy of the NDT,
// host_score_points(); (2) the few candidates of a marked near-tie are rescored in the
// reference's own arithmetic, settle_near_tie().  Every search, every batch of poses and every
// longer scan is evaluated on the GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "host/ndt2d_matcher_state.h"
#include "ndt2d_guard.h"

using namespace ndt2d::host;

// ---- what the other units of the matcher use (host/ndt2d_matcher_state.h) ----

void ndt2d::host::fill_rotations(ndt2d_matcher * m, double scan_theta)
{
  const size_t n_th = m->search.dth.size();
  m->search.cos_th.resize(n_th);
  m->search.sin_th.resize(n_th);
  for (size_t i = 0; i < n_th; ++i) ndt2d_cos_sin(scan_theta + m->search.dth[i], &m->search.cos_th[i], &m->search.sin_th[i]);
}

size_t ndt2d::host::adopt_scan(ndt2d_matcher * m, const double * points_xy, size_t n_points, bool * held_out)
{
  subsample_into(m->beams.next, points_xy, n_points, m->laser_max_beams);
  const size_t use = m->beams.next.size() / 2;
  const bool held = m->beams.holds(m->beams.next);
  if (!held) m->beams.adopt(m->beams.next);   // (the host copy; the context's beams stay)
  m->search.n_use = use;
  m->search.ready = false;
  if (held_out != nullptr) *held_out = held;
  return use;
}

namespace
{

// ROS angles::normalize_angle / shortest_angular_distance (unpinned dependency
// of the reference, used by updateStatistics src/particle_filter.cpp:215).
double normalize_angle(double a)
{
  const double r = std::fmod(a + M_PI, 2.0 * M_PI);
  return r <= 0.0 ? r + M_PI : r - M_PI;
}

// The visited offsets of the search and the per-theta cos/sin (reference
// src/scan_matcher_ndt.cpp:103-107,117,119).  host_beams != nullptr: they are uploaded
// together with the beams in one copy; nullptr: the beams are on the device already
// (LaserScan conversion) and only the tables travel.
int prepare_tables(ndt2d_matcher * m, const double * scan_pose_xyt, size_t use,
                   const double * host_beams, bool beams_cached, size_t * n_th_out,
                   size_t * n_lin_out)
{
  // (the visited offsets depend on the parameters only: computed by initialize())
  const size_t n_th = m->search.dth.size(), n_lin = m->search.dlin.size();
  if (n_th_out != nullptr) *n_th_out = n_th;
  if (n_lin_out != nullptr) *n_lin_out = n_lin;
  m->search.ready = false;
  if (use == 0 || n_th == 0 || n_lin == 0 || !m->ndt.have()) return NDT2D_OK;  // nothing to upload

  fill_rotations(m, scan_pose_xyt[2]);
  int rc;
  if (host_beams != nullptr || beams_cached)
  {
    rc = ndt2d_set_search_beams(m->dev, host_beams, use, scan_pose_xyt[0], scan_pose_xyt[1],
                                m->search.dth.data(), m->search.cos_th.data(), m->search.sin_th.data(), n_th,
                                m->search.dlin.data(), n_lin);
    if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_set_search_beams");
    m->beams.sent();
  }
  else
  {
    rc = ndt2d_set_search(m->dev, scan_pose_xyt[0], scan_pose_xyt[1], m->search.dth.data(),
                          m->search.cos_th.data(), m->search.sin_th.data(), n_th, m->search.dlin.data(), n_lin);
    if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_set_search");
  }
  m->search.ready = true;
  return NDT2D_OK;
}

// The host copy of the beams to the first device.
int upload_beams(ndt2d_matcher * m)
{
  const int rc = ndt2d_set_beams(m->dev, m->beams.host.data(), m->beams.host.size() / 2);
  if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_set_beams");
  m->beams.sent();
  return NDT2D_OK;
}

// Subsample `points` (src/scan_matcher_ndt.cpp:165-166,171) and make them the device
// context's beams -- unless they are exactly what it holds already.  *use_out = beams.
// pending_out != nullptr: a changed scan is only adopted (*pending_out = true): the caller
// hands m->beams.host to ndt2d_score_poses_beams, which uploads it or passes it along as
// kernel arguments.
int stage_beams(ndt2d_matcher * m, const double * points_xy, size_t n_points, size_t * use_out,
                bool * pending_out = nullptr)
{
  if (pending_out != nullptr) *pending_out = false;
  subsample_into(m->beams.next, points_xy, n_points, m->laser_max_beams);
  const size_t use = m->beams.next.size() / 2;
  *use_out = use;
  if (use == 0 || m->beams.holds(m->beams.next)) return NDT2D_OK;   // (same scan as the last call: the beams are there)
  m->search.ready = false;  // the device beams are replaced: a prepared search is void
  m->beams.adopt(m->beams.next);
  if (pending_out == nullptr) return upload_beams(m);
  *pending_out = true;
  return NDT2D_OK;
}

// Is the search launched ahead still the one pending on the context?  (A caller may have launched
// or fetched on ndt2d_matcher_device(m) itself in between: then the record is not ours.)
bool ahead_on_context(ndt2d_matcher * m)
{
  uint64_t launched = 0, fetched = 0;
  return ndt2d_match_status(m->dev, &launched, &fetched) == NDT2D_OK && launched == m->ahead.launch_id &&
         fetched == m->ahead.fetch_id;
}

// A search launched ahead that the call now arriving cannot use: wait it out (its record is
// dropped), and do not launch ahead again until the scoreScan / matchScan pair reappears.
}  // namespace

void ndt2d::host::discard_ahead(ndt2d_matcher * m)
{
  m->ahead.after_score_scan = false;
  if (!m->ahead.pending) return;
  if (ahead_on_context(m))
  {
    ndt2d_match_result res;
    (void)ndt2d_match_fetch(m->dev, &res);
  }
  m->ahead.pending = false;
  m->ahead.pair_seen = false;
}

namespace
{

// ... and forget the pair even when nothing was pending (the lattice or the switch changed).
void forget_ahead(ndt2d_matcher * m)
{
  discard_ahead(m);
  m->ahead.pair_seen = false;
}

// scoreScan: the prepared search of its scan launched now, for the matchScan that follows to
// collect.  (A search that cannot be launched is not scoreScan's failure: matchScan will say.)
void launch_ahead(ndt2d_matcher * m, const double * scan_pose_xyt, size_t n_th, size_t use)
{
  if (!m->search.ready || ndt2d_match_launch(m->dev, 0, n_th, nullptr, nullptr) != NDT2D_OK) return;
  ndt2d_matcher::SearchAhead & a = m->ahead;
  a.pending = true;
  (void)ndt2d_match_status(m->dev, &a.launch_id, &a.fetch_id);
  ++a.launched;
  std::memcpy(a.pose, scan_pose_xyt, sizeof(a.pose));
  a.n_th = n_th;
  m->search.n_use = use;
}

// matchScan: the search launched ahead, if it is this call's -- no per-candidate scores wanted,
// the pose bitwise the same, the same subsampled beams, still the search pending on the context --
// fetched into `record` (marked: record_from), *n_th_out = its theta steps.  Any other search
// launched ahead is discarded (*n_th_out = 0).
int collect_ahead(ndt2d_matcher * m, const double * scan_pose_xyt, const double * points_xy, size_t n_points,
                  bool want_scores, double * record, size_t * n_th_out)
{
  ndt2d_matcher::SearchAhead & a = m->ahead;
  *n_th_out = 0;
  if (!a.pending) return NDT2D_OK;
  bool hit = !want_scores && (n_points == 0 || points_xy != nullptr) &&
             std::memcmp(a.pose, scan_pose_xyt, sizeof(a.pose)) == 0;
  if (hit)
  {
    subsample_into(m->beams.next, points_xy, n_points, m->laser_max_beams);
    hit = m->beams.holds(m->beams.next) && ahead_on_context(m);
  }
  if (!hit)
  {
    discard_ahead(m);
    return NDT2D_OK;
  }
  a.pending = false;
  a.after_score_scan = false;
  ++a.collected;
  *n_th_out = a.n_th;
  ndt2d_match_result res;
  const int rc = ndt2d_match_fetch(m->dev, &res);
  if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_match_fetch");
  record_from(res, record);
  return NDT2D_OK;
}

// scoreScan of this pose and scan answered: the matchScan after it may be of the same.
void note_score_scan(ndt2d_matcher * m, const double * scan_pose_xyt, const double * points_xy, size_t n_points)
{
  ndt2d_matcher::SearchAhead & a = m->ahead;
  a.after_score_scan = true;
  std::memcpy(a.score_scan_pose, scan_pose_xyt, sizeof(a.score_scan_pose));
  subsample_into(a.scored, points_xy, n_points, m->laser_max_beams);
}

// matchScan (prepared: its search was prepared, m->beams.host holds its subsampled beams): the
// pair is seen when it is of the scan and pose the scoreScan just before it scored.
void note_match_scan(ndt2d_matcher * m, const double * scan_pose_xyt, bool prepared)
{
  ndt2d_matcher::SearchAhead & a = m->ahead;
  if (prepared && a.after_score_scan && std::memcmp(a.score_scan_pose, scan_pose_xyt, sizeof(a.score_scan_pose)) == 0 &&
      same_beams(m->beams.host, a.scored))
  {
    a.pair_seen = true;
  }
  a.after_score_scan = false;
}

// scorePoints / scoreScan: one pose of a short scan, scored on the host (ndt2d_matcher_set_single_pose_path)?
bool single_pose_on_host(const ndt2d_matcher * m, const double * points_xy, size_t n_points)
{
  return m->single_pose_host && !m->ndt.fused() && m->ndt.have() && n_points > 0 && points_xy != nullptr && m->laser_max_beams > 0 &&
         std::min(m->laser_max_beams, n_points) <= m->single_pose_max_beams;
}

// The host NDT the single-pose path and the near-tie adjudication score against: the one
// addScans built on the host, or -- for a grid built on the DEVICE (maps of 73,728 points and
// more) -- its records fetched back once per addScans.  That fetch is the whole dense grid
// (48 bytes per cell, synchronous) plus a host pool of the same size: worth it for the grids
// the single-pose path exists for, not for a loop-closure map of a million cells, where it
// would cost tens of megabytes over PCIe to save a 30 us launch.  for_single_pose: the caller
// can take the device path instead, so a grid above kHostFetchMaxCells is left on the device;
// the adjudication of a marked near-tie (rare, and it has no device path) fetches any size.
// nullptr also when memory runs out -- nothing may throw through the C-ABI.
constexpr size_t kHostFetchMaxCells = 65536;   // 3 MB of records

const HostNdt * host_ndt(ndt2d_matcher * m, bool for_single_pose)
{
  if (const HostNdt * have = m->ndt.host_copy()) return have;
  uint32_t sx = 0, sy = 0;
  double cs = 0.0, ox = 0.0, oy = 0.0;
  if (ndt2d_get_grid(m->dev, nullptr, 0, &sx, &sy, &cs, &ox, &oy) != NDT2D_OK) return nullptr;
  const size_t ncell = static_cast<size_t>(sx) * sy;
  if (for_single_pose && ncell > kHostFetchMaxCells) return nullptr;
  try
  {
    std::vector<double> cells(ncell * 6);
    if (ndt2d_get_grid(m->dev, cells.data(), ncell, nullptr, nullptr, nullptr, nullptr, nullptr) != NDT2D_OK)
    {
      return nullptr;
    }
    std::unique_ptr<HostNdt> g(new HostNdt(cs, 0.0, 0.0, ox, oy));
    g->reset_cells(cs, sx, sy, ox, oy);
    g->load6(cells.data());
    return m->ndt.fetched_back(std::move(g));
  }
  catch (const std::bad_alloc &)
  {
    return nullptr;
  }
}

// ScanMatcherNDT::scorePoints on the host (reference src/scan_matcher_ndt.cpp:156-178): the
// pose as toEigen makes it (conversions.hpp:64-68: [[c, -s], [s, c]] and the translation),
// the subsampling of :165-171, `score += -likelihood(p)` in beam order, score / N.
double host_score_points(const HostNdt & ndt, const double * points_xy, size_t n_points, size_t laser_max_beams,
                         const double * pose_xyt)
{
  double c, s;
  ndt2d_cos_sin(pose_xyt[2], &c, &s);
  const size_t use = std::min(laser_max_beams, n_points);
  const double scan_step = static_cast<double>(n_points) / use;
  double score = 0.0;
  for (size_t i = 0; i < use; ++i)
  {
    const size_t idx = static_cast<size_t>(i * scan_step);
    const double x = points_xy[2 * idx], y = points_xy[2 * idx + 1];
    const double px = pose_xyt[0] + (c * x + (-s) * y);
    const double py = pose_xyt[1] + (s * x + c * y);
    score += -ndt.likelihood(px, py);
  }
  return score / use;
}

// One candidate of matchScan's lattice as the reference scores it (src/scan_matcher_ndt.cpp:
// 106-127): points_outer from the subsampled beams (m->beams.host) and cos/sin of
// scan_pose.theta + dth, points_inner = outer + (dx, dy), score = -(likelihoods summed in order).
double host_score_candidate(const HostNdt & ndt, const double * beams_xy, size_t use, const double * scan_pose_xyt,
                            double costh, double sinth, double dx, double dy)
{
  double sum = 0.0;
  for (size_t i = 0; i < use; ++i)
  {
    const double bx = beams_xy[2 * i], by = beams_xy[2 * i + 1];
    const double ox = bx * costh - by * sinth + scan_pose_xyt[0];
    const double oy = bx * sinth + by * costh + scan_pose_xyt[1];
    sum += ndt.likelihood(ox + dx, oy + dy);
  }
  return -sum;
}

// A search's record came back with its winner marked (index + 0.5: another candidate within
// the near-tie tolerance, ndt2d_device_fn.h merge_best): list the candidates that close to the best,
// rescore them as the reference would and apply its rule -- strict `<` in visiting order
// (src/scan_matcher_ndt.cpp:128-134).  The first device holds the prepared search.  record[1]
// leaves here as a plain index.
int settle_near_tie(ndt2d_matcher * m, const double * scan_pose_xyt, size_t n_th, size_t n_lin, size_t use, double * record)
{
  if (!marked_winner(record)) return NDT2D_OK;
  record[1] = std::floor(record[1]);
  ++m->adj_marked;
  if (!m->adjudicate || m->beams.host.size() != 2 * use || m->search.cos_th.size() != n_th) return NDT2D_OK;
  const HostNdt * ndt = host_ndt(m, false);
  if (ndt == nullptr) return NDT2D_OK;
  constexpr size_t kCap = 256;
  uint64_t idx[kCap + 1];
  size_t n = 0;
  const int rc = ndt2d_match_near_best(m->dev, 0, n_th, NDT2D_NEAR_TIE_REL, idx, kCap, &n, nullptr);
  if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_match_near_best");
  if (n > kCap) ++m->adj_truncated;
  size_t listed = std::min(n, kCap);
  // The device's own winner is always among the rescored: a plateau of more than kCap
  // candidates is cut to the first kCap in visiting order, and the winner may lie beyond the
  // cut -- it must then not be replaced by a candidate that neither the device nor the
  // reference would pick (only by one whose reference-order score is strictly lower).
  {
    const uint64_t winner = static_cast<uint64_t>(record[1]);
    uint64_t * const end = idx + listed;
    uint64_t * const at = std::lower_bound(idx, end, winner);
    if (at == end || *at != winner)
    {
      const size_t pos = static_cast<size_t>(at - idx);
      for (size_t k = listed; k > pos; --k) idx[k] = idx[k - 1];
      idx[pos] = winner;
      ++listed;
    }
  }
  const uint64_t per_th = static_cast<uint64_t>(n_lin) * n_lin;
  double best_s = 0.0;   // `double best_score = 0;` (:83)
  uint64_t best_i = NDT2D_NO_INDEX;
  for (size_t k = 0; k < listed; ++k)   // ascending flat index = the reference's visiting order
  {
    const uint64_t ith = idx[k] / per_th, rem = idx[k] % per_th;
    if (ith >= n_th) continue;
    const double score = host_score_candidate(*ndt, m->beams.host.data(), use, scan_pose_xyt, m->search.cos_th[ith],
                                              m->search.sin_th[ith], m->search.dlin[rem / n_lin], m->search.dlin[rem % n_lin]);
    if (score < best_s)
    {
      best_s = score;
      best_i = idx[k];
    }
  }
  if (best_i != NDT2D_NO_INDEX)
  {
    if (static_cast<double>(best_i) != record[1]) ++m->adj_changed;
    record[0] = best_s;
    record[1] = static_cast<double>(best_i);
  }
  return NDT2D_OK;
}
void destroy_matcher(ndt2d_matcher * m)
{
  m->workers.reset();   // (the threads end before the contexts they drive)
  // (a matcher whose creation failed half-way has contexts but no shard records yet)
  for (size_t r = 0; r < m->devs.size() && r < m->shards.size(); ++r)
  {
    MatcherShard & sh = m->shards[r];
    (void)ndt2d_synchronize(m->devs[r]);
    if (sh.d_table != nullptr) ndt2d_device_free(m->devs[r], sh.d_table);
    if (sh.d_sum != nullptr) ndt2d_device_free(m->devs[r], sh.d_sum);
    if (sh.d_scores != nullptr) ndt2d_device_free(m->devs[r], sh.d_scores);
    if (sh.d_poses != nullptr) ndt2d_device_free(m->devs[r], sh.d_poses);
    if (sh.d_weights != nullptr) ndt2d_device_free(m->devs[r], sh.d_weights);
  }
  if (m->closure != nullptr) (void)ndt2d_closure_destroy(m->closure);         // (before its store)
  if (m->starts != nullptr) (void)ndt2d_starts_destroy(m->starts);            // (before its context)
  if (m->wide != nullptr) (void)ndt2d_wide_destroy(m->wide);                  // (before its context)
  if (m->scans != nullptr) (void)ndt2d_scans_destroy(m->scans);               // (before its context)
  if (m->refine != nullptr) (void)ndt2d_refine_destroy(m->refine);            // (before its context)
  if (m->verify != nullptr) (void)ndt2d_verify_destroy(m->verify);            // (before its context)
  for (ndt2d_scanstore * st : m->stores) (void)ndt2d_scanstore_destroy(st);   // (before their contexts)
  for (ndt2d_handle h : m->devs) (void)ndt2d_build_small_release(h);
  if (m->exchange != nullptr) ndt2d::exchange_destroy(m->exchange);
  if (m->pinned != nullptr && !m->devs.empty()) ndt2d_host_free(m->dev, m->pinned);
  for (ndt2d_handle h : m->devs) ndt2d_destroy(h);
  delete m;
}

}  // namespace

extern "C" {

int ndt2d_matcher_create_multi(ndt2d_matcher ** out, const int * device_ids, int n_dev)
{
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (device_ids == nullptr || n_dev <= 0 || n_dev > 64) return NDT2D_ERR_INVALID;
  ndt2d_matcher * m = new (std::nothrow) ndt2d_matcher();
  if (m == nullptr) return NDT2D_ERR_ALLOC;
  try
  {
    m->devs.reserve(static_cast<size_t>(n_dev));
    m->device_ids.reserve(static_cast<size_t>(n_dev));
    for (int r = 0; r < n_dev; ++r)
    {
      ndt2d_handle dev = nullptr;
      const int rc = ndt2d_create(&dev, device_ids[r]);
      if (rc != NDT2D_OK)
      {
        destroy_matcher(m);
        return rc;
      }
      m->devs.push_back(dev);
      m->device_ids.push_back(device_ids[r]);
    }
    m->shards.resize(m->devs.size());
    m->dev = m->devs[0];
    m->workers.reset(new ndt2d::DeviceWorkers(m->devs.size()));
    m->search.dth = search_offsets(m->angular_size, m->angular_res);
    m->search.dlin = search_offsets(m->linear_size, m->linear_res);
  }
  catch (const std::bad_alloc &)
  {
    destroy_matcher(m);
    return NDT2D_ERR_ALLOC;
  }
  catch (...)
  {
    destroy_matcher(m);
    return NDT2D_ERR_INTERNAL;   // (no thread could be started)
  }
  *out = m;
  return NDT2D_OK;
}

int ndt2d_matcher_create(ndt2d_matcher ** out, int device_id)
{
  NDT2D_C_TRY
  return ndt2d_matcher_create_multi(out, &device_id, 1);
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_matcher_destroy(ndt2d_matcher * m)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  discard_ahead(m);
  destroy_matcher(m);
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_device_count(ndt2d_matcher * m) { return m != nullptr ? static_cast<int>(m->devs.size()) : 0; }

ndt2d_handle ndt2d_matcher_device_at(ndt2d_matcher * m, int rank)
{
  return (m != nullptr && rank >= 0 && static_cast<size_t>(rank) < m->devs.size()) ? m->devs[static_cast<size_t>(rank)] : nullptr;
}

int ndt2d_matcher_set_exchange(ndt2d_matcher * m, const char * mode)
{
  NDT2D_C_TRY
  if (m == nullptr || mode == nullptr) return NDT2D_ERR_INVALID;
  if (std::strcmp(mode, "auto") == 0) m->exchange_mode = 0;
  else if (std::strcmp(mode, "host") == 0) m->exchange_mode = 1;
  else if (std::strcmp(mode, "rccl") == 0) m->exchange_mode = 2;
  else return mfail(m, NDT2D_ERR_INVALID, "set_exchange: unknown mode (auto, host, rccl)");
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_multi_min_units(ndt2d_matcher * m, double units)
{
  NDT2D_C_TRY
  return ndt2d_matcher_set_multi_thresholds(m, units, units);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_multi_thresholds(ndt2d_matcher * m, double min_search_units, double min_pose_units)
{
  NDT2D_C_TRY
  if (m == nullptr || !(min_search_units >= 0.0) || !(min_pose_units >= 0.0)) return NDT2D_ERR_INVALID;
  m->multi_min_units = min_search_units;
  m->multi_min_pose_units = min_pose_units;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_get_multi_thresholds(ndt2d_matcher * m, double * min_search_units, double * min_pose_units)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (min_search_units != nullptr) *min_search_units = m->multi_min_units;
  if (min_pose_units != nullptr) *min_pose_units = m->multi_min_pose_units;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_last_fanout_us(ndt2d_matcher * m, double * out_us, size_t capacity, size_t * n_out)
{
  NDT2D_C_TRY
  if (m == nullptr || (capacity > 0 && out_us == nullptr)) return NDT2D_ERR_INVALID;
  if (n_out != nullptr) *n_out = m->fanout_us.size();
  for (size_t r = 0; r < m->fanout_us.size() && r < capacity; ++r) out_us[r] = m->fanout_us[r];
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

const char * ndt2d_matcher_last_variant(ndt2d_matcher * m)
{
  if (m == nullptr) return "";
  try
  {
    if (!m->last_multi) note_variant(m, false, false);   // whatever the first device ran last
  }
  catch (...)
  {
    return "";
  }
  return m->variant.c_str();
}

int ndt2d_matcher_set_timing(ndt2d_matcher * m, int enabled)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  for (ndt2d_handle h : m->devs)
  {
    const int rc = ndt2d_set_timing(h, enabled);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

const char * ndt2d_matcher_last_error(ndt2d_matcher * m)
{
  return m != nullptr ? m->err.c_str() : "null matcher";
}

ndt2d_handle ndt2d_matcher_device(ndt2d_matcher * m) { return m != nullptr ? m->dev : nullptr; }

int ndt2d_matcher_initialize(ndt2d_matcher * m, double ndt_resolution,
                             double search_angular_resolution, double search_angular_size,
                             double search_linear_resolution, double search_linear_size,
                             size_t laser_max_beams, double range_max)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (!(ndt_resolution > 0.0) || !std::isfinite(ndt_resolution))
  {
    return mfail(m, NDT2D_ERR_INVALID, "ndt_resolution must be a finite number > 0");
  }
  if (!std::isfinite(range_max)) return mfail(m, NDT2D_ERR_INVALID, "range_max must be finite");
  // The lattice is visited by `for (v = -size; v < size; v += res)` (src/scan_matcher_ndt.cpp:103,
  // 117,119): a step the range never gets past would not end there, and one that needs more steps
  // than a search can take (ndt2d_set_search: 2^24 angular, 46,340 linear) would only fill memory
  // here -- refused before a single offset is stored.
  if (!offsets_fit(search_angular_size, search_angular_resolution, 1u << 24) ||
      !offsets_fit(search_linear_size, search_linear_resolution, 46340))
  {
    return mfail(m, NDT2D_ERR_INVALID, "search lattice: size / resolution must be finite, the resolution > 0, at most "
                                       "2^24 angular and 46,340 linear steps");
  }
  forget_ahead(m);
  m->resolution = ndt_resolution;
  m->angular_res = search_angular_resolution;
  m->angular_size = search_angular_size;
  m->linear_res = search_linear_resolution;
  m->linear_size = search_linear_size;
  m->laser_max_beams = laser_max_beams;
  m->range_max = range_max;
  m->search.dth = search_offsets(m->angular_size, m->angular_res);
  m->search.dlin = search_offsets(m->linear_size, m->linear_res);
  m->search.ready = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_add_scans(ndt2d_matcher * m, const double * poses_xyt,
                            const double * points_xy, const size_t * offsets, size_t n_scans)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_scans > 0 && (poses_xyt == nullptr || offsets == nullptr))
  {
    return mfail(m, NDT2D_ERR_INVALID, "add_scans: null input");
  }
  for (size_t k = 0; k < 3 * n_scans; ++k)
  {
    if (!std::isfinite(poses_xyt[k])) return mfail(m, NDT2D_ERR_INVALID, "add_scans: a scan pose is not finite");
  }
  for (size_t k = 0; k < n_scans; ++k)
  {
    if (offsets[k + 1] < offsets[k]) return mfail(m, NDT2D_ERR_INVALID, "add_scans: offsets must not decrease");
  }
  discard_ahead(m);
  static const double no_points[2] = {0.0, 0.0};
  if (points_xy == nullptr) points_xy = no_points;
  static const size_t no_offsets[1] = {0};
  if (offsets == nullptr) offsets = no_offsets;
  std::unique_ptr<HostNdt> storage = m->ndt.begin_build();   // no NDT is in place from here on
  // Device build (N1): the whole of addScans on the GPU, bit-identical to the host
  // build; "auto" uses it from kDeviceBuildFromPoints map points up, where it beats the host build
  // (round 5, whole addScans call, host / device: 0.068 / 0.134 ms at 6,480 points, 0.192 / 0.252
  // at 32,400, 0.324 / 0.340 at 64,800, 0.409 / 0.346 at 86,400, 0.64 / 0.44 at 144,000, 1.72 /
  // 0.79 at 378,000 -- experiments/build_crossover.py; the device build is ~130 us of launches
  // and a synchronisation plus 3.4 ns per point, the host build 40 us plus 4.4 ns per point).
  constexpr size_t kDeviceBuildFromPoints = 73728;   // ~100 scans of 720 beams (32,768 until round 5)
  const size_t n_map_points = n_scans > 0 ? offsets[n_scans] : 0;
  // "fused" (opt-in): the one-workgroup build for maps within its limits, otherwise as "auto"
  const bool fused = n_scans > 0 && m->build_mode == 3 &&
                     ndt2d_build_grid_small_fits(m->resolution, m->range_max, poses_xyt, n_scans, n_map_points) != 0;
  const bool on_device =
    n_scans > 0 && (fused || m->build_mode == 2 ||
                    ((m->build_mode == 0 || m->build_mode == 3) && n_map_points >= kDeviceBuildFromPoints));
  if (on_device)
  {
    storage.reset();
    // (every device of a multi-device matcher builds its own copy: the builds run side by side)
    for (size_t r = 0; r < m->devs.size(); ++r)
    {
      int rc;
      if (fused)
      {
        // (the fused build keeps its eigenvalue form beside the context: handed over with every build)
        rc = ndt2d_build_small_set_eigenvalue_form(m->devs[r], eigen_form_name(m));
        if (rc == NDT2D_OK)
        {
          rc = ndt2d_build_grid_small(m->devs[r], m->resolution, m->range_max, poses_xyt, points_xy, offsets, n_scans);
        }
      }
      else
      {
        rc = ndt2d_build_grid(m->devs[r], m->resolution, m->range_max, poses_xyt, points_xy, offsets, n_scans);
      }
      if (rc != NDT2D_OK)
      {
        return m->ndt.give_up(m->devs, fused ? mfail(m, rc, "ndt2d_build_grid_small (rank " + std::to_string(r) + "): " +
                                                              ndt2d_build_small_last_error(m->devs[r]))
                                             : dev_fail_at(m, r, rc, "ndt2d_build_grid"));
      }
    }
    m->ndt.built_on_device(fused);
    return NDT2D_OK;
  }
  std::unique_ptr<HostNdt> ndt = build_ndt(m->resolution, m->range_max, poses_xyt, points_xy, offsets, n_scans,
                                           std::move(storage), m->eigen_form);
  if (!ndt || ndt->ncell() == 0)
  {
    return m->ndt.give_up(m->devs, mfail(m, NDT2D_ERR_INVALID, "add_scans: degenerate grid extent (scan poses +- range_max "
                                                               "must span a finite grid of fewer than 2^31 cells)"));
  }
  // The cells that hold points travel, not the grid (ndt2d_set_grid_sparse: the install kernel
  // reads the staged list in place, two launches and no copy; 245 x 245 cells: 297 us dense ->
  // 29 us per addScans, and at 41 x 41 the list is ahead as well: 34 -> 32 us plus 7 us less
  // for the stream to be ready for the call that follows, experiments/cycle_breakdown.c).
  // (written straight into the library's pinned staging buffer: ndt2d_grid_stage_begin / _commit)
  for (size_t r = 0; r < m->devs.size(); ++r)
  {
    uint32_t * list_index = nullptr;
    double * list_cells6 = nullptr;
    int rc = ndt2d_grid_stage_begin(m->devs[r], static_cast<uint32_t>(ndt->size_x()),
                                    static_cast<uint32_t>(ndt->size_y()), ndt->n_touched(), &list_index,
                                    &list_cells6);
    if (rc == NDT2D_OK)
    {
      ndt->sparse6(list_index, list_cells6);
      rc = ndt2d_grid_stage_commit(m->devs[r], ndt->n_touched(), ndt->cell_size(), ndt->origin_x(),
                                   ndt->origin_y());
    }
    if (rc != NDT2D_OK) return m->ndt.give_up(m->devs, dev_fail_at(m, r, rc, "ndt2d_set_grid"));
  }
  m->ndt.built_on_host(std::move(ndt));
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_eigenvalue_form(ndt2d_matcher * m, const char * form)
{
  NDT2D_C_TRY
  if (m == nullptr || form == nullptr) return NDT2D_ERR_INVALID;
  for (ndt2d_handle h : m->devs)
  {
    const int rc = ndt2d_set_eigenvalue_form(h, form);
    if (rc != NDT2D_OK) return mfail(m, rc, "set_eigenvalue_form: unknown form (eigen, closed)");
  }
  m->eigen_form = std::strcmp(form, "closed") == 0 ? ndt2d::kEigenFormClosed : ndt2d::kEigenFormSchur;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_build_mode(ndt2d_matcher * m, const char * mode)
{
  NDT2D_C_TRY
  if (m == nullptr || mode == nullptr) return NDT2D_ERR_INVALID;
  if (std::strcmp(mode, "auto") == 0) m->build_mode = 0;
  else if (std::strcmp(mode, "host") == 0) m->build_mode = 1;
  else if (std::strcmp(mode, "device") == 0) m->build_mode = 2;
  else if (std::strcmp(mode, "fused") == 0) m->build_mode = 3;
  else return mfail(m, NDT2D_ERR_INVALID, "set_build_mode: unknown mode");
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

// Resident scans: what one device's store holds (the mapper's rolling window is ten scans, a
// loop closure's candidates a few dozen; 4 MB of points per device).
static constexpr size_t kStorePoints = 262144, kStoreScans = 4096;

int ndt2d_matcher_store_scan(ndt2d_matcher * m, const double * points_xy, size_t n_points, size_t * id_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_points > 0 && points_xy == nullptr) return mfail(m, NDT2D_ERR_INVALID, "store_scan: null points");
  while (m->stores.size() < m->devs.size())
  {
    const size_t r = m->stores.size();
    ndt2d_scanstore * st = nullptr;
    const int rc = ndt2d_scanstore_create(m->devs[r], kStorePoints, kStoreScans, &st);
    if (rc != NDT2D_OK) return dev_fail_at(m, r, rc, "ndt2d_scanstore_create");
    m->stores.push_back(st);
  }
  size_t id = 0;
  for (size_t r = 0; r < m->stores.size(); ++r)
  {
    size_t id_r = 0;
    const int rc = ndt2d_scanstore_append(m->stores[r], points_xy, n_points, &id_r);
    if (rc != NDT2D_OK)
    {
      const std::string why = ndt2d_scanstore_last_error(m->stores[r]);
      // (a full store refuses on the first device, before any holds the scan; a copy that failed on a
      // later one would leave the stores with different ids: they all start over)
      if (r > 0) for (ndt2d_scanstore * st : m->stores) (void)ndt2d_scanstore_reset(st);
      return mfail(m, rc, "store_scan (rank " + std::to_string(r) + "): " + why +
                            (r > 0 ? "; every stored scan was dropped" : ""));
    }
    if (r == 0) id = id_r;
  }
  if (id_out != nullptr) *id_out = id;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_add_scans_by_id(ndt2d_matcher * m, const double * poses_xyt, const size_t * ids, size_t n_scans)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_scans == 0 || poses_xyt == nullptr || ids == nullptr)
  {
    return mfail(m, NDT2D_ERR_INVALID, "add_scans_by_id: null input");
  }
  for (size_t k = 0; k < 3 * n_scans; ++k)
  {
    if (!std::isfinite(poses_xyt[k])) return mfail(m, NDT2D_ERR_INVALID, "add_scans_by_id: a scan pose is not finite");
  }
  if (m->stores.size() != m->devs.size()) return mfail(m, NDT2D_ERR_INVALID, "add_scans_by_id: unknown scan id (no scan is stored)");
  discard_ahead(m);
  // (every device builds its own copy from its own store, as add_scans replicates builds)
  for (size_t r = 0; r < m->devs.size(); ++r)
  {
    int rc = ndt2d_scanstore_set_eigenvalue_form(m->stores[r], eigen_form_name(m));
    if (rc == NDT2D_OK) rc = ndt2d_scanstore_build(m->stores[r], ids, poses_xyt, n_scans, m->resolution, m->range_max);
    if (rc != NDT2D_OK)
    {
      const int frc = mfail(m, rc, "add_scans_by_id (rank " + std::to_string(r) + "): " +
                                     ndt2d_scanstore_last_error(m->stores[r]));
      // a refusal comes from the first store before anything is launched: the NDT in place stays
      return (r == 0 && rc == NDT2D_ERR_INVALID) ? frc : m->ndt.give_up(m->devs, frc);
    }
    // the grid is replaced from here on: no host NDT, as after a device build
    if (r == 0) m->ndt.begin_build().reset();
  }
  m->ndt.built_on_device(true);
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

const char * ndt2d_matcher_last_build(ndt2d_matcher * m) { return m != nullptr ? m->ndt.last_build() : ""; }

int ndt2d_matcher_drop_scans(ndt2d_matcher * m)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  for (ndt2d_scanstore * st : m->stores) (void)ndt2d_scanstore_reset(st);
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_reset(ndt2d_matcher * m)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  discard_ahead(m);
  return m->ndt.drop(m->devs);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_has_ndt(ndt2d_matcher * m) { return (m != nullptr && m->ndt.have()) ? 1 : 0; }

static int prepare_search_impl(ndt2d_matcher * m, const double * scan_pose_xyt,
                               const double * points_xy, size_t n_points, size_t * n_th_out,
                               size_t * n_lin_out, size_t * n_beams_out)
{
  if (m == nullptr || scan_pose_xyt == nullptr) return NDT2D_ERR_INVALID;
  if (n_points > 0 && points_xy == nullptr) return mfail(m, NDT2D_ERR_INVALID, "null points");
  // the scan scoreScan was just called with (src/ndt_mapper.cpp:514-515)?  Then the
  // device holds these beams already and only the tables are new.
  bool same = false;
  const size_t use = adopt_scan(m, points_xy, n_points, &same);
  if (n_beams_out != nullptr) *n_beams_out = use;
  return prepare_tables(m, scan_pose_xyt, use, same ? nullptr : m->beams.host.data(), same, n_th_out,
                        n_lin_out);
}

int ndt2d_matcher_prepare_search(ndt2d_matcher * m, const double * scan_pose_xyt,
                                 const double * points_xy, size_t n_points, size_t * n_th_out,
                                 size_t * n_lin_out, size_t * n_beams_out)
{
  NDT2D_C_TRY
  if (m != nullptr) discard_ahead(m);
  return prepare_search_impl(m, scan_pose_xyt, points_xy, n_points, n_th_out, n_lin_out, n_beams_out);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_finish_match(ndt2d_matcher * m, const double * record, double * pose_inout,
                               double * covariance_out, double * score_out)
{
  NDT2D_C_TRY
  if (m == nullptr || record == nullptr || score_out == nullptr) return NDT2D_ERR_INVALID;
  // n_use is the N of the search prepared last (prepare_search / match_laser_scan);
  // scoring calls in between replace the device beams but leave it alone
  const size_t use = m->search.n_use;
  const size_t n_lin = m->search.dlin.size();
  const double best_score = record[0];
  if (record[1] >= 0.0 && pose_inout != nullptr && n_lin > 0)
  {
    // reference src/scan_matcher_ndt.cpp:128-134: pose = the accumulated
    // offsets of the winning candidate
    const uint64_t best_index = static_cast<uint64_t>(record[1]);   // (truncates a near-tie mark, index + 0.5)
    const uint64_t per_th = static_cast<uint64_t>(n_lin) * n_lin;
    const uint64_t ith = best_index / per_th;
    const uint64_t rem = best_index % per_th;
    if (ith >= m->search.dth.size()) return mfail(m, NDT2D_ERR_INVALID, "finish_match: index out of range");
    pose_inout[0] = m->search.dlin[rem / n_lin];
    pose_inout[1] = m->search.dlin[rem % n_lin];
    pose_inout[2] = m->search.dth[ith];
  }
  // :146 covariance = (1 / s) * k + (1 / (s * s) * u * u^T)
  if (covariance_out != nullptr)
  {
    const double * k = record + 2;
    const double * u = record + 8;
    const double s = record[11];
    const double kk[9] = {k[0], k[1], k[2], k[1], k[3], k[4], k[2], k[4], k[5]};
    const double inv_s = 1 / s;
    const double inv_s2 = 1 / (s * s);
    for (int r = 0; r < 3; ++r)
    {
      for (int c = 0; c < 3; ++c)
      {
        covariance_out[r * 3 + c] = inv_s * kk[r * 3 + c] + (inv_s2 * u[r]) * u[c];
      }
    }
  }
  // :148
  *score_out = best_score / use;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_match_scan_ex(ndt2d_matcher * m, const double * scan_pose_xyt,
                                const double * points_xy, size_t n_points,
                                double * pose_inout, double * covariance_out,
                                double * score_out, double * all_scores,
                                size_t all_scores_cap, size_t * n_candidates_out,
                                uint64_t * best_index_out)
{
  NDT2D_C_TRY
  if (m == nullptr || score_out == nullptr || scan_pose_xyt == nullptr)
  {
    return NDT2D_ERR_INVALID;
  }
  if (n_candidates_out != nullptr) *n_candidates_out = 0;
  if (best_index_out != nullptr) *best_index_out = NDT2D_NO_INDEX;
  // `if (!ndt_) return 0.0;` (reference src/scan_matcher_ndt.cpp:80): outputs untouched
  if (!m->ndt.have())
  {
    *score_out = 0.0;
    return NDT2D_OK;
  }
  m->last_multi = false;
  // record = {best_score, best_index or -1, k00,k01,k02,k11,k12,k22, u0,u1,u2, s}
  double record[NDT2D_MATCH_RECORD_DOUBLES] = {0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  size_t n_th = 0, n_lin = m->search.dlin.size(), use = m->search.n_use;
  std::vector<double> tmp;
  int rc = collect_ahead(m, scan_pose_xyt, points_xy, n_points, all_scores != nullptr, record, &n_th);
  if (n_th > 0)
  {
    // the search scoreScan launched ahead for this call
    if (n_candidates_out != nullptr) *n_candidates_out = n_th * n_lin * n_lin;
    if (rc != NDT2D_OK) return rc;
  }
  else
  {
    rc = prepare_search_impl(m, scan_pose_xyt, points_xy, n_points, &n_th, &n_lin, &use);
    note_match_scan(m, scan_pose_xyt, rc == NDT2D_OK);
    if (rc != NDT2D_OK) return rc;
    const size_t n_cand = n_th * n_lin * n_lin;
    if (n_candidates_out != nullptr) *n_candidates_out = n_cand;
    if (!m->search.ready)
    {
      // No points: every candidate scores -0.0 and none is < 0 (:127-128); no
      // candidates: the loops do not run.  Either way k = u = s = 0.
      for (size_t i = 0; all_scores != nullptr && i < n_cand && i < all_scores_cap; ++i) all_scores[i] = -0.0;
      return ndt2d_matcher_finish_match(m, record, pose_inout, covariance_out, score_out);
    }
    double * scores_ptr = all_scores;
    if (all_scores != nullptr && all_scores_cap < n_cand)
    {
      tmp.resize(n_cand);
      scores_ptr = tmp.data();
    }
    if ((rc = run_search(m, scan_pose_xyt, n_th, n_lin, use, false, scores_ptr, record)) != NDT2D_OK) return rc;
  }
  if ((rc = settle_near_tie(m, scan_pose_xyt, n_th, n_lin, use, record)) != NDT2D_OK) return rc;
  if (!tmp.empty()) std::memcpy(all_scores, tmp.data(), all_scores_cap * sizeof(double));
  if (best_index_out != nullptr) *best_index_out = record_best_index(record);
  return ndt2d_matcher_finish_match(m, record, pose_inout, covariance_out, score_out);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_match_scan(ndt2d_matcher * m, const double * scan_pose_xyt,
                             const double * points_xy, size_t n_points, double * pose_inout,
                             double * covariance_out, double * score_out)
{
  NDT2D_C_TRY
  return ndt2d_matcher_match_scan_ex(m, scan_pose_xyt, points_xy, n_points, pose_inout,
                                     covariance_out, score_out, nullptr, 0, nullptr, nullptr);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_match_laser_scan(ndt2d_matcher * m, const double * scan_pose_xyt,
                                   const float * ranges, size_t n_ranges,
                                   const ndt2d_laser_scan * scan, double * pose_inout,
                                   double * covariance_out, double * score_out,
                                   size_t * n_points_out)
{
  NDT2D_C_TRY
  if (m == nullptr || score_out == nullptr || scan_pose_xyt == nullptr || scan == nullptr)
  {
    return NDT2D_ERR_INVALID;
  }
  if (n_ranges > 0 && ranges == nullptr) return mfail(m, NDT2D_ERR_INVALID, "null ranges");
  if (n_points_out != nullptr) *n_points_out = 0;
  // `if (!ndt_) return 0.0;` (reference src/scan_matcher_ndt.cpp:80): outputs untouched
  if (!m->ndt.have())
  {
    *score_out = 0.0;
    return NDT2D_OK;
  }
  discard_ahead(m);
  size_t n_points = 0, use = 0;
  ranges = off_grid_ranges(m->scratch_ranges, ranges, n_ranges, scan->range_max);
  int rc = ndt2d_set_beams_from_ranges(m->dev, ranges, n_ranges, scan, m->laser_max_beams,
                                       &n_points, &use);
  if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_set_beams_from_ranges");
  if (n_points_out != nullptr) *n_points_out = n_points;
  std::vector<double> none;
  m->beams.adopt(none);   // the device holds beams the host has no copy of
  m->search.n_use = use;
  size_t n_th = 0, n_lin = 0;
  rc = prepare_tables(m, scan_pose_xyt, use, nullptr, false, &n_th, &n_lin);
  if (rc != NDT2D_OK) return rc;
  double record[NDT2D_MATCH_RECORD_DOUBLES] = {0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  m->last_multi = false;
  if (m->search.ready)
  {
    if (multi_search_wanted(m, n_th, n_lin, use))
    {
      // every device converts the ranges itself (4 B/beam to each), then takes its theta steps
      for (size_t r = 1; r < m->devs.size(); ++r)
      {
        size_t np = 0, nu = 0;
        rc = ndt2d_set_beams_from_ranges(m->devs[r], ranges, n_ranges, scan, m->laser_max_beams, &np, &nu);
        if (rc != NDT2D_OK) return dev_fail_at(m, r, rc, "ndt2d_set_beams_from_ranges");
        if (np != n_points || nu != use) return mfail(m, NDT2D_ERR_HIP, "match_laser_scan: the devices disagree on the conversion");
      }
    }
    if ((rc = run_search(m, scan_pose_xyt, n_th, n_lin, use, true, nullptr, record)) != NDT2D_OK) return rc;
    // (no host copy of the converted beams: a near-tie mark is counted, not settled)
    if (marked_winner(record)) ++m->adj_marked;
    if (record[1] >= 0.0) record[1] = std::floor(record[1]);
  }
  return ndt2d_matcher_finish_match(m, record, pose_inout, covariance_out, score_out);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_score_poses(ndt2d_matcher * m, const double * points_xy, size_t n_points,
                              const double * poses_xyt, size_t n_poses, double * scores_out)
{
  NDT2D_C_TRY
  if (m == nullptr || scores_out == nullptr || (n_poses > 0 && poses_xyt == nullptr))
  {
    return NDT2D_ERR_INVALID;
  }
  if (n_poses == 0) return NDT2D_OK;
  discard_ahead(m);
  // `if (!ndt_) return 0.0;` (reference src/scan_matcher_ndt.cpp:159)
  if (!m->ndt.have())
  {
    for (size_t i = 0; i < n_poses; ++i) scores_out[i] = 0.0;
    return NDT2D_OK;
  }
  if (n_points > 0 && points_xy == nullptr) return mfail(m, NDT2D_ERR_INVALID, "null points");
  size_t use = 0;
  bool pending = false;
  int rc = stage_beams(m, points_xy, n_points, &use, &pending);
  if (rc != NDT2D_OK) return rc;
  if (use == 0)
  {
    // score = 0.0 / 0 (:177)
    for (size_t i = 0; i < n_poses; ++i) scores_out[i] = std::numeric_limits<double>::quiet_NaN();
    return NDT2D_OK;
  }
  m->last_multi = false;
  if (multi_poses_wanted(m, n_poses, use))
  {
    // contiguous ranges of the batch on all devices of the matcher
    if (pending && (rc = upload_beams(m)) != NDT2D_OK) return rc;
    return multi_score_poses(m, poses_xyt, n_poses, use, scores_out, nullptr);
  }
  if (pending)
  {
    // a new scan: its beams go to the device with the scoring call itself
    rc = ndt2d_score_poses_beams(m->dev, m->beams.host.data(), use, poses_xyt, n_poses, scores_out);
    if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_score_poses_beams");
    m->beams.sent();
    return NDT2D_OK;
  }
  rc = ndt2d_score_poses(m->dev, poses_xyt, n_poses, scores_out, nullptr);
  if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_score_poses");
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_prepare_beams(ndt2d_matcher * m, const double * points_xy, size_t n_points,
                                size_t * n_beams_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_points > 0 && points_xy == nullptr) return mfail(m, NDT2D_ERR_INVALID, "null points");
  discard_ahead(m);
  size_t use = 0;
  int rc = stage_beams(m, points_xy, n_points, &use);
  if (n_beams_out != nullptr) *n_beams_out = use;
  return rc;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_score_points(ndt2d_matcher * m, const double * points_xy, size_t n_points,
                               const double * pose_xyt, double * score_out)
{
  NDT2D_C_TRY
  if (pose_xyt == nullptr || score_out == nullptr) return NDT2D_ERR_INVALID;
  if (m != nullptr && single_pose_on_host(m, points_xy, n_points))
  {
    // One pose of a short scan -- the unchanged ParticleFilter::measure calls this once per
    // particle (reference src/particle_filter.cpp:81-87): a kernel launch and a round trip over
    // PCIe per call would cost several times the arithmetic, so the host scores it, from the host
    // NDT, in the reference's order ("the unchanged node + unchanged ParticleFilter
    // keep working via per-pose scorePoints").  Nothing on the device is touched: a search
    // launched ahead by scoreScan stays pending.
    if (const HostNdt * ndt = host_ndt(m, true))
    {
      *score_out = host_score_points(*ndt, points_xy, n_points, m->laser_max_beams, pose_xyt);
      return NDT2D_OK;
    }
  }
  return ndt2d_matcher_score_poses(m, points_xy, n_points, pose_xyt, 1, score_out);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_score_scan(ndt2d_matcher * m, const double * scan_pose_xyt,
                             const double * points_xy, size_t n_points, double * score_out)
{
  NDT2D_C_TRY
  // scoreScan(scan) = scorePoints(scan->getPoints(), scan->getPose()) (:151-154)
  if (m == nullptr || scan_pose_xyt == nullptr || score_out == nullptr) return NDT2D_ERR_INVALID;
  discard_ahead(m);
  m->last_multi = false;
  const bool ahead_wanted = m->ahead.enabled && m->ahead.pair_seen && m->ndt.have() &&
                            (n_points == 0 || points_xy != nullptr) && !m->search.dth.empty() && !m->search.dlin.empty() &&
                            !multi_search_wanted(m, m->search.dth.size(), m->search.dlin.size(),
                                                 std::min(m->laser_max_beams, n_points));
  if (single_pose_on_host(m, points_xy, n_points))
  {
    if (const HostNdt * ndt = host_ndt(m, true))
    {
      // The host scores the pose (see ndt2d_matcher_score_points) -- and when the matchScan of
      // this scan is coming (SearchAhead), its search is launched first and runs meanwhile.
      if (ahead_wanted)
      {
        size_t n_th = 0, n_lin = 0, use = 0;
        if (prepare_search_impl(m, scan_pose_xyt, points_xy, n_points, &n_th, &n_lin, &use) == NDT2D_OK)
        {
          launch_ahead(m, scan_pose_xyt, n_th, use);
        }
      }
      *score_out = host_score_points(*ndt, points_xy, n_points, m->laser_max_beams, scan_pose_xyt);
      note_score_scan(m, scan_pose_xyt, points_xy, n_points);
      return NDT2D_OK;
    }
  }
  if (ahead_wanted)
  {
    // The matchScan of this scan is coming (SearchAhead): its search goes onto the stream
    // behind the scoring kernel, then the score is waited for.
    size_t use = 0;
    bool pending = false;
    int rc = stage_beams(m, points_xy, n_points, &use, &pending);
    if (rc != NDT2D_OK) return rc;
    if (use > 0)
    {
      rc = ndt2d_score_poses_beams_launch(m->dev, pending ? m->beams.host.data() : nullptr, use, scan_pose_xyt, 1);
      if (rc == NDT2D_ERR_STATE && pending)
      {
        // more beams than travel as kernel arguments: one staged upload, then the launch on
        // the beams the device holds
        if ((rc = upload_beams(m)) != NDT2D_OK) return rc;
        rc = ndt2d_score_poses_beams_launch(m->dev, nullptr, use, scan_pose_xyt, 1);
      }
      if (rc == NDT2D_OK)
      {
        m->beams.sent();
        size_t n_th = 0, n_lin = 0;
        if (prepare_tables(m, scan_pose_xyt, use, nullptr, true, &n_th, &n_lin) == NDT2D_OK)
        {
          launch_ahead(m, scan_pose_xyt, n_th, use);
        }
        rc = ndt2d_score_fetch(m->dev, score_out);
        if (rc != NDT2D_OK)
        {
          const int frc = dev_fail(m, rc, "ndt2d_score_fetch");   // (the message, before anything else talks to the device)
          discard_ahead(m);
          m->beams.lost();
          return frc;
        }
        note_score_scan(m, scan_pose_xyt, points_xy, n_points);
        return NDT2D_OK;
      }
      if (rc != NDT2D_ERR_STATE) return dev_fail(m, rc, "ndt2d_score_poses_beams_launch");
      // (not a kernel-argument launch -- more beams than travel as arguments: the ordinary call)
    }
  }
  const int rc = ndt2d_matcher_score_poses(m, points_xy, n_points, scan_pose_xyt, 1, score_out);
  if (rc == NDT2D_OK && m->ndt.have()) note_score_scan(m, scan_pose_xyt, points_xy, n_points);
  return rc;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_settle_near_tie(ndt2d_matcher * m, const double * scan_pose_xyt, double * record_inout)
{
  NDT2D_C_TRY
  if (m == nullptr || scan_pose_xyt == nullptr || record_inout == nullptr) return NDT2D_ERR_INVALID;
  if (!m->search.ready) return mfail(m, NDT2D_ERR_STATE, "settle_near_tie: ndt2d_matcher_prepare_search first");
  discard_ahead(m);
  return settle_near_tie(m, scan_pose_xyt, m->search.dth.size(), m->search.dlin.size(), m->search.n_use, record_inout);
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_adjudication(ndt2d_matcher * m, int enabled)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  m->adjudicate = enabled != 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_adjudication_stats(ndt2d_matcher * m, uint64_t * marked, uint64_t * changed, uint64_t * truncated)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (marked != nullptr) *marked = m->adj_marked;
  if (changed != nullptr) *changed = m->adj_changed;
  if (truncated != nullptr) *truncated = m->adj_truncated;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_single_pose_path(ndt2d_matcher * m, const char * where, size_t max_beams)
{
  NDT2D_C_TRY
  if (m == nullptr || where == nullptr) return NDT2D_ERR_INVALID;
  if (std::strcmp(where, "host") == 0) m->single_pose_host = true;
  else if (std::strcmp(where, "device") == 0) m->single_pose_host = false;
  else return mfail(m, NDT2D_ERR_INVALID, "set_single_pose_path: unknown path (host, device)");
  if (max_beams > 0) m->single_pose_max_beams = max_beams;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_search_ahead_stats(ndt2d_matcher * m, uint64_t * launched, uint64_t * collected)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (launched != nullptr) *launched = m->ahead.launched;
  if (collected != nullptr) *collected = m->ahead.collected;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_search_ahead(ndt2d_matcher * m, int enabled)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  forget_ahead(m);
  m->ahead.enabled = enabled != 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_pf_measure(ndt2d_matcher * m, const double * particles_xyt,
                             size_t n_particles, const double * points_xy, size_t n_points,
                             double * weights_out, double * mean_out, double * cov_inout)
{
  NDT2D_C_TRY
  if (m == nullptr || weights_out == nullptr || mean_out == nullptr || cov_inout == nullptr ||
      (n_particles > 0 && particles_xyt == nullptr))
  {
    return NDT2D_ERR_INVALID;
  }
  discard_ahead(m);
  if (n_particles > 0 && m->ndt.have() && n_points > 0 && m->laser_max_beams > 0)
  {
    // weights_[i] = scorePoints(points, particle_i) (particle_filter.cpp:81-87), then
    // updateStatistics (:163-218), all on the device
    if (points_xy == nullptr) return mfail(m, NDT2D_ERR_INVALID, "null points");
    size_t use = 0;
    int rc = stage_beams(m, points_xy, n_points, &use);
    if (rc != NDT2D_OK) return rc;
    double out[NDT2D_PF_RESULT_DOUBLES];
    m->last_multi = false;
    if (multi_poses_wanted(m, n_particles, use))
    {
      rc = multi_score_poses(m, particles_xyt, n_particles, use, weights_out, out);
      if (rc != NDT2D_OK) return rc;
    }
    else
    {
      rc = ndt2d_pf_measure(m->dev, particles_xyt, n_particles, weights_out, out);
      if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_pf_measure");
    }
    mean_out[0] = out[1];
    mean_out[1] = out[2];
    mean_out[2] = out[3];
    cov_inout[0] = out[4];
    cov_inout[1] = out[5];
    cov_inout[3] = out[5];
    cov_inout[4] = out[6];
    cov_inout[8] += out[7];  // cov_(2,2) accumulates (:216)
    return NDT2D_OK;
  }

  // Degenerate inputs (no map / no points / no particles): every weight is the
  // constant scorePoints returns (0.0 or NaN); the statistics of those constants.
  if (n_particles > 0)
  {
    int rc = ndt2d_matcher_score_poses(m, points_xy, n_points, particles_xyt, n_particles,
                                       weights_out);
    if (rc != NDT2D_OK) return rc;
  }
  double stats[NDT2D_POSE_STATS_DOUBLES] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t i = 0; i < n_particles; ++i)
  {
    const double w = weights_out[i];
    const double * p = particles_xyt + 3 * i;
    stats[0] += w;
    stats[1] += w * p[0];
    stats[2] += w * p[1];
    double cos_p, sin_p;
    ndt2d_cos_sin(p[2], &cos_p, &sin_p);
    stats[3] += w * cos_p;
    stats[4] += w * sin_p;
    stats[5] += w * p[0] * p[0];
    stats[6] += w * p[0] * p[1];
    stats[7] += w * p[1] * p[1];
  }
  const double sum_weight = stats[0];
  for (size_t i = 0; i < n_particles; ++i) weights_out[i] /= sum_weight;
  const double mean_x = stats[1] / sum_weight;
  const double mean_y = stats[2] / sum_weight;
  mean_out[0] = mean_x;
  mean_out[1] = mean_y;
  mean_out[2] = std::atan2(stats[4] / sum_weight, stats[3] / sum_weight);
  cov_inout[0] = stats[5] / sum_weight - mean_x * mean_x;
  cov_inout[1] = stats[6] / sum_weight - mean_x * mean_y;
  cov_inout[3] = cov_inout[1];
  cov_inout[4] = stats[7] / sum_weight - mean_y * mean_y;
  for (size_t i = 0; i < n_particles; ++i)
  {
    const double d = normalize_angle(mean_out[2] - particles_xyt[3 * i + 2]);
    cov_inout[8] += weights_out[i] * d * d;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_grid_info(ndt2d_matcher * m, uint32_t * size_x, uint32_t * size_y,
                            double * cell_size, double * origin_x, double * origin_y)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (!m->ndt.have()) return mfail(m, NDT2D_ERR_NO_GRID, "no NDT");
  int rc = ndt2d_get_grid(m->dev, nullptr, 0, size_x, size_y, cell_size, origin_x, origin_y);
  return rc == NDT2D_OK ? rc : dev_fail(m, rc, "ndt2d_get_grid");
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_grid_cells6(ndt2d_matcher * m, double * cells6_out, size_t capacity_cells)
{
  NDT2D_C_TRY
  if (m == nullptr || cells6_out == nullptr) return NDT2D_ERR_INVALID;
  if (!m->ndt.have()) return mfail(m, NDT2D_ERR_NO_GRID, "no NDT");
  discard_ahead(m);
  if (const HostNdt * built = m->ndt.built())
  {
    if (capacity_cells < built->ncell()) return mfail(m, NDT2D_ERR_INVALID, "capacity too small");
    built->pack6(cells6_out);
    return NDT2D_OK;
  }
  int rc = ndt2d_get_grid(m->dev, cells6_out, capacity_cells, nullptr, nullptr, nullptr, nullptr,
                          nullptr);
  return rc == NDT2D_OK ? rc : dev_fail(m, rc, "ndt2d_get_grid");
  NDT2D_C_CATCH(m)
}

}  // extern "C"
