// The three batched matches of the matcher -- a scan against all its candidate maps
// (match_candidates), from K start poses (match_starts), K scans each from its own pose (match_scans):
// each validates its input, makes one call of its object under csrc/closure, starts or scans for
// the records of all slots, and hands them to finish_slots(), the tail they share -- and the Newton
// registration of K (scan, pose) jobs (refine_scans), one call of the object under csrc/refine, and
// the same on each loop-closure candidate's own map (refine_candidates), one call of the closure object,
// and the match verification of K (scan, pose) jobs (verify_scans), one call of the object under csrc/verify,
// and the same on each loop-closure candidate's own map (verify_candidates), one call of the closure object.
// The five calls on a (scan, pose) job list check it, collect its batch and deal the records back through
// host/ndt2d_job_batch.h.
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "host/ndt2d_job_batch.h"
#include "host/ndt2d_matcher_state.h"
#include "ndt2d_guard.h"

using namespace ndt2d::host;

namespace
{

constexpr size_t kRec = NDT2D_MATCH_RECORD_DOUBLES;

// `if (!ndt_) return 0.0;` (reference src/scan_matcher_ndt.cpp:80) for every slot: the other outputs untouched
void fill_no_ndt(size_t n, double * scores_out, uint64_t * best_index_out)
{
  for (size_t k = 0; k < n; ++k)
  {
    scores_out[k] = 0.0;
    if (best_index_out != nullptr) best_index_out[k] = NDT2D_NO_INDEX;
  }
}

// all_scores is filled only where it takes the lattice of every slot
double * scores_if_they_fit(double * all_scores, size_t all_scores_cap, size_t n_slots, size_t n_lattice)
{
  return (all_scores != nullptr && all_scores_cap / n_slots >= n_lattice && n_lattice > 0) ? all_scores : nullptr;
}

// Slot k's part of the caller's output arrays ...
struct SlotOut
{
  double * pose, * covariance, * score;
  uint64_t * best_index;
  double * lattice_scores;
};

// ... which are these (poses, covariances, best indices and lattice scores are optional: scores_if_they_fit)
struct BatchOut
{
  double * poses, * covariances, * scores;
  uint64_t * best_index;
  double * lattice_scores;
  size_t n_lattice;
  SlotOut slot(size_t k) const
  {
    return {poses != nullptr ? poses + 3 * k : nullptr, covariances != nullptr ? covariances + 9 * k : nullptr, scores + k,
            best_index != nullptr ? best_index + k : nullptr, lattice_scores != nullptr ? lattice_scores + k * n_lattice : nullptr};
  }
};

// The sequential call of one slot: matchScan of `points` from `scan_pose_xyt` into the slot's outputs.
int match_alone(ndt2d_matcher * m, const double * scan_pose_xyt, const double * points_xy, size_t n_points,
                const SlotOut & o, size_t n_lattice)
{
  return ndt2d_matcher_match_scan_ex(m, scan_pose_xyt, points_xy, n_points, o.pose, o.covariance, o.score, o.lattice_scores,
                                     n_lattice, nullptr, o.best_index);
}

// The tail of a batched match: slot k's record (records[k]) becomes its best index, pose, covariance and
// score -- unless sequential[k]: a marked winner (index + 0.5), whose adjudication the sequential call
// settles, or a batch without points or lattice (every candidate scores -0.0 and none is < 0; the loops
// do not run), of which the sequential call says what it gives.  alone(k, out) is that call;
// set_n(k), if any, sets the N of `best / N` (:148) before a record is finished.  The first failure
// ends the loop, its text prefixed with `slot_name` and the slot.
int finish_slots(ndt2d_matcher * m, size_t n_slots, const double * records, const std::vector<char> & sequential,
                 const BatchOut & out, const char * slot_name, const std::function<int(size_t, const SlotOut &)> & alone,
                 const std::function<void(size_t)> & set_n = nullptr)
{
  int rc = NDT2D_OK;
  for (size_t k = 0; k < n_slots && rc == NDT2D_OK; ++k)
  {
    const SlotOut o = out.slot(k);
    if (sequential[k])
    {
      rc = alone(k, o);
      if (rc != NDT2D_OK) m->err = slot_name + std::to_string(k) + ": " + m->err;
      continue;
    }
    if (set_n) set_n(k);
    const double * rec = records + k * kRec;
    if (o.best_index != nullptr) *o.best_index = record_best_index(rec);
    rc = ndt2d_matcher_finish_match(m, rec, o.pose, o.covariance, o.score);
  }
  return rc;
}

// Candidates the batched match launches at a time: the plugin's global_search_limit_ is a handful.
constexpr size_t kClosureSlots = 16;

// The registration's rules, as refine_scans and refine_candidates take them.
struct RefineRules
{
  uint32_t max_evals;
  double tol_lin, tol_ang;
};

// What the batched calls on a job list refuse about its size, the rules (NULL: a verification, which
// has none), the scans and the jobs, in that order; `who` names the call.
int check_job_input(ndt2d_matcher * m, const std::string & who, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                    const double * points_xy, const size_t * point_offsets, size_t n_scans, const RefineRules * rules)
{
  std::string refusal = job_list_size_refusal(who, n_jobs, n_scans);
  if (refusal.empty() && rules != nullptr)
  {
    if (rules->max_evals == 0) refusal = who + ": max_evals == 0";
    else if (!(rules->tol_lin >= 0.0) || !(rules->tol_ang >= 0.0) || !std::isfinite(rules->tol_lin) || !std::isfinite(rules->tol_ang))
    {
      refusal = who + ": a tolerance is negative or not finite";
    }
  }
  if (refusal.empty()) refusal = job_list_refusal(who, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans);
  return refusal.empty() ? NDT2D_OK : mfail(m, NDT2D_ERR_INVALID, refusal);
}

// What refine_candidates and verify_candidates refuse about the jobs' candidates; `who` names the call.
int check_job_candidates(ndt2d_matcher * m, const std::string & who, const uint32_t * job_candidate, size_t n_jobs,
                         size_t n_candidates)
{
  if (job_candidate == nullptr && n_candidates != n_jobs)
  {
    return mfail(m, NDT2D_ERR_INVALID, who + ": no job_candidate (job k uses candidate k): n_candidates must equal n_jobs");
  }
  for (size_t k = 0; k < n_jobs && job_candidate != nullptr; ++k)
  {
    if (job_candidate[k] >= n_candidates)
    {
      return mfail(m, NDT2D_ERR_INVALID, who + ": job " + std::to_string(k) + ": candidate " + std::to_string(job_candidate[k]) +
                                             " of " + std::to_string(n_candidates));
    }
  }
  if (m->stores.size() != m->devs.size()) return mfail(m, NDT2D_ERR_INVALID, who + ": candidate 0: unknown scan id (no scan is stored)");
  return NDT2D_OK;
}

// `if (!ndt_) return 0.0;` (src/scan_matcher_ndt.cpp:159), and a scan without points: nothing
// scores, the job keeps its pose
void fill_no_overlap(const double * jobs_xyt, size_t n_jobs, const RefineOut & o)
{
  for (size_t k = 0; k < n_jobs; ++k)
  {
    std::memcpy(o.poses + 3 * k, jobs_xyt + 3 * k, 3 * sizeof(double));
    o.scores[k] = 0.0;
    o.status[k] = NDT2D_REFINE_NO_OVERLAP;
    if (o.start_scores != nullptr) o.start_scores[k] = 0.0;
    if (o.gradients != nullptr) std::memset(o.gradients + 3 * k, 0, 3 * sizeof(double));
    if (o.hessians != nullptr) std::memset(o.hessians + 9 * k, 0, 9 * sizeof(double));
    if (o.evals != nullptr) o.evals[2 * k] = o.evals[2 * k + 1] = 0u;
  }
}

// The candidates of the batch's jobs; job_candidate NULL: job k uses candidate k.
std::vector<uint32_t> batch_candidates(const JobBatch & batch, const uint32_t * job_candidate)
{
  std::vector<uint32_t> out(batch.size());
  for (size_t j = 0; j < batch.size(); ++j) out[j] = job_candidate != nullptr ? job_candidate[batch.job[j]] : batch.job[j];
  return out;
}

// The closure object, made by the first call that needs it.
int ensure_closure(ndt2d_matcher * m)
{
  if (m->closure != nullptr) return NDT2D_OK;
  const int rc = ndt2d_closure_create(m->dev, m->stores[0], kClosureSlots, &m->closure);
  return rc == NDT2D_OK ? NDT2D_OK : dev_fail(m, rc, "ndt2d_closure_create");
}

// Where a verification's results go (verify_scans, verify_candidates); all but records are optional.
struct VerifyOut
{
  uint32_t * records;
  size_t * beam_offsets;
  uint8_t * beam_class;
  double * beam_m2;
  uint32_t * beam_cells;
  size_t beam_cap;
};

// What both verifications do round their device call: the capacity refusal, the zeroed records and
// the offsets table of all n_jobs jobs -- before the device call (fill_first) or only after it
// succeeded --, the call on a batch that has jobs, and its records dealt to their jobs.
// run(records): the device call into [batch job][NDT2D_VERIFY_RECORD_U32]; the per-beam arrays are
// the batch's, job after job: a job without beams takes no room in them.
template <class RUN>
int verify_batch(ndt2d_matcher * m, const std::string & who, const JobBatch & batch, size_t n_jobs, const VerifyOut & out,
                 bool fill_first, RUN run)
{
  const size_t n_beams_all = batch_beams(batch);
  const bool want_beams = out.beam_class != nullptr || out.beam_m2 != nullptr || out.beam_cells != nullptr;
  if (want_beams && out.beam_cap < n_beams_all)
  {
    return mfail(m, NDT2D_ERR_INVALID, who + ": the per-beam arrays hold " + std::to_string(out.beam_cap) + " beams, the jobs have " +
                                           std::to_string(n_beams_all));
  }
  const auto fill = [&]() {
    std::memset(out.records, 0, n_jobs * NDT2D_VERIFY_RECORD_U32 * sizeof(uint32_t));   // (the jobs of a scan without points keep this)
    if (out.beam_offsets != nullptr) fill_verify_offsets(batch, n_jobs, out.beam_offsets);
  };
  if (fill_first) fill();
  std::vector<uint32_t> records(batch.size() * NDT2D_VERIFY_RECORD_U32);
  if (batch.size() != 0)
  {
    const int rc = run(records.data());
    if (rc != NDT2D_OK) return rc;
  }
  if (!fill_first) fill();
  deal_verify_records(batch, records.data(), NDT2D_VERIFY_RECORD_U32, out.records);
  return NDT2D_OK;
}

}  // namespace

extern "C" {

int ndt2d_matcher_match_candidates(ndt2d_matcher * m, const double * scan_pose_xyt, const double * points_xy,
                                   size_t n_points, const size_t * cand_offsets, const size_t * ids,
                                   const double * poses_xyt, size_t n_candidates, double * poses_out,
                                   double * covariances_out, double * scores_out, uint64_t * best_index_out,
                                   double * all_scores, size_t all_scores_cap, size_t * n_lattice_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (scan_pose_xyt == nullptr || scores_out == nullptr || (n_points > 0 && points_xy == nullptr) ||
      (n_candidates > 0 && (cand_offsets == nullptr || ids == nullptr || poses_xyt == nullptr)))
  {
    return mfail(m, NDT2D_ERR_INVALID, "match_candidates: null input");
  }
  const size_t n_th = m->search.dth.size(), n_lin = m->search.dlin.size();
  const size_t n_lattice = n_th * n_lin * n_lin;
  if (n_lattice_out != nullptr) *n_lattice_out = n_lattice;
  if (n_candidates == 0) return NDT2D_OK;
  if (n_candidates > (1u << 20)) return mfail(m, NDT2D_ERR_INVALID, "match_candidates: too many candidates");
  if (m->stores.size() != m->devs.size())
  {
    return mfail(m, NDT2D_ERR_INVALID, "match_candidates: candidate 0: unknown scan id (no scan is stored)");
  }
  discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
  const int crc = ensure_closure(m);
  if (crc != NDT2D_OK) return crc;
  double * scores_ptr = scores_if_they_fit(all_scores, all_scores_cap, n_candidates, n_lattice);

  // the scan as matchScan takes it: subsampled beams (:95-96,110), cos / sin per theta step (:106-107)
  const size_t use = adopt_scan(m, points_xy, n_points);
  fill_rotations(m, scan_pose_xyt[2]);
  m->closure_records.assign(n_candidates * kRec, 0.0);
  double * records = m->closure_records.data();
  std::vector<char> sequential(n_candidates, 1);   // (no points, or no lattice: every slot)
  if (use > 0 && n_lattice > 0)
  {
    int rc = ndt2d_scanstore_set_eigenvalue_form(m->stores[0], eigen_form_name(m));
    if (rc == NDT2D_OK)
    {
      rc = ndt2d_closure_match(m->closure, n_candidates, cand_offsets, ids, poses_xyt, m->resolution, m->range_max,
                               m->beams.host.data(), use, scan_pose_xyt[0], scan_pose_xyt[1], m->search.dth.data(),
                               m->search.cos_th.data(), m->search.sin_th.data(), n_th, m->search.dlin.data(), n_lin,
                               records, scores_ptr);
    }
    if (rc != NDT2D_OK) return mfail(m, rc, std::string("match_candidates: ") + ndt2d_closure_last_error(m->closure));
    for (size_t k = 0; k < n_candidates; ++k) sequential[k] = marked_winner(records + k * kRec);
  }
  const BatchOut out = {poses_out, covariances_out, scores_out, best_index_out, scores_ptr, n_lattice};
  const auto alone = [&](size_t k, const SlotOut & o) {
    // the candidate's map built as the loop would build it, then matchScan
    const size_t j0 = cand_offsets[k], n_k = cand_offsets[k + 1] - cand_offsets[k];
    int rc = ndt2d_matcher_reset(m);
    if (rc == NDT2D_OK) rc = ndt2d_matcher_add_scans_by_id(m, poses_xyt + 3 * j0, ids + j0, n_k);
    return rc == NDT2D_OK ? match_alone(m, scan_pose_xyt, points_xy, n_points, o, n_lattice) : rc;
  };
  const int rc = finish_slots(m, n_candidates, records, sequential, out, "match_candidates: candidate ", alone);
  // `global_scan_matcher_->reset()` (src/ndt_mapper.cpp:634): no NDT is left in place
  const int rrc = ndt2d_matcher_reset(m);
  return rc != NDT2D_OK ? rc : rrc;
  NDT2D_C_CATCH(m)
}

ndt2d_closure * ndt2d_matcher_closure(ndt2d_matcher * m) { return m != nullptr ? m->closure : nullptr; }

// Starts the batched match launches at a time: the object's limit (a relocalisation over every
// graph node under a few headings is hundreds to a few thousand).
static constexpr size_t kStartsSlots = 4096;

int ndt2d_matcher_match_starts(ndt2d_matcher * m, const double * starts_xyt, size_t n_starts, const double * points_xy,
                               size_t n_points, double * poses_out, double * covariances_out, double * scores_out,
                               uint64_t * best_index_out, double * all_scores, size_t all_scores_cap,
                               size_t * n_lattice_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_lattice_out != nullptr) *n_lattice_out = 0;
  if (n_starts == 0) return NDT2D_OK;
  if (starts_xyt == nullptr || scores_out == nullptr || (n_points > 0 && points_xy == nullptr))
  {
    return mfail(m, NDT2D_ERR_INVALID, "match_starts: null input");
  }
  if (n_starts > (1u << 20)) return mfail(m, NDT2D_ERR_INVALID, "match_starts: too many starts");
  if (!m->ndt.have())
  {
    fill_no_ndt(n_starts, scores_out, best_index_out);
    return NDT2D_OK;
  }
  for (size_t k = 0; k < n_starts; ++k)
  {
    if (!std::isfinite(starts_xyt[3 * k]) || !std::isfinite(starts_xyt[3 * k + 1]) || !std::isfinite(starts_xyt[3 * k + 2]))
    {
      return mfail(m, NDT2D_ERR_INVALID, "match_starts: start " + std::to_string(k) + ": the pose is not finite");
    }
  }
  const size_t n_th = m->search.dth.size(), n_lin = m->search.dlin.size();
  const size_t n_lattice = n_th * n_lin * n_lin;
  if (n_lattice_out != nullptr) *n_lattice_out = n_lattice;
  discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
  if (m->starts == nullptr)
  {
    const int rc = ndt2d_starts_create(m->dev, kStartsSlots, &m->starts);
    if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_starts_create");
  }
  double * scores_ptr = scores_if_they_fit(all_scores, all_scores_cap, n_starts, n_lattice);

  // the scan as matchScan takes it: subsampled beams (:95-96,110), once for every start
  const size_t use = adopt_scan(m, points_xy, n_points);
  m->starts_records.assign(n_starts * kRec, 0.0);
  double * records = m->starts_records.data();
  std::vector<char> sequential(n_starts, 1);   // (no points, or no lattice: every slot)
  if (use > 0 && n_lattice > 0)
  {
    const int rc = ndt2d_starts_match(m->starts, starts_xyt, n_starts, m->beams.host.data(), use, m->search.dth.data(), n_th,
                                      m->search.dlin.data(), n_lin, records, scores_ptr);
    if (rc != NDT2D_OK) return mfail(m, rc, std::string("match_starts: ") + ndt2d_starts_last_error(m->starts));
    m->last_multi = false;
    for (size_t k = 0; k < n_starts; ++k) sequential[k] = marked_winner(records + k * kRec);
  }
  const BatchOut out = {poses_out, covariances_out, scores_out, best_index_out, scores_ptr, n_lattice};
  return finish_slots(
    m, n_starts, records, sequential, out, "match_starts: start ",
    [&](size_t k, const SlotOut & o) { return match_alone(m, starts_xyt + 3 * k, points_xy, n_points, o, n_lattice); },
    // (a sequential call prepared a search of its own; the records after it are finished with this N)
    [&](size_t) { m->search.n_use = use; });
  NDT2D_C_CATCH(m)
}

ndt2d_starts * ndt2d_matcher_starts(ndt2d_matcher * m) { return m != nullptr ? m->starts : nullptr; }

// Tile jobs the wide search scores in one launch at most (its chunks double up to this).
static constexpr size_t kWideMaxTiles = size_t(1) << 16;

int ndt2d_matcher_match_wide(ndt2d_matcher * m, const double * scan_pose_xyt, const double * points_xy, size_t n_points,
                             double linear_size, double linear_res, double angular_size, double angular_res,
                             uint32_t tile_steps, double * pose_out, double * score_out, uint64_t * best_index_out,
                             int * near_tie_out, uint64_t * stats_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (scan_pose_xyt == nullptr || score_out == nullptr || (n_points > 0 && points_xy == nullptr))
  {
    return mfail(m, NDT2D_ERR_INVALID, "match_wide: null input");
  }
  *score_out = 0.0;
  if (best_index_out != nullptr) *best_index_out = NDT2D_NO_INDEX;
  if (near_tie_out != nullptr) *near_tie_out = 0;
  if (stats_out != nullptr) stats_out[0] = stats_out[1] = 0;
  // `if (!ndt_) return 0.0;` (reference src/scan_matcher_ndt.cpp:80)
  if (!m->ndt.have()) return NDT2D_OK;
  if (!std::isfinite(scan_pose_xyt[0]) || !std::isfinite(scan_pose_xyt[1]) || !std::isfinite(scan_pose_xyt[2]))
  {
    return mfail(m, NDT2D_ERR_INVALID, "match_wide: a non-finite scan pose");
  }
  if (!offsets_fit(linear_size, linear_res, 46340) || !offsets_fit(angular_size, angular_res, 1u << 24))
  {
    return mfail(m, NDT2D_ERR_INVALID, "match_wide: the sizes and resolutions give no lattice ndt2d_set_search takes");
  }
  const std::vector<double> dlin = search_offsets(linear_size, linear_res), dth = search_offsets(angular_size, angular_res);
  discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
  // the scan as matchScan takes it: subsampled beams (:95-96,110)
  const size_t use = adopt_scan(m, points_xy, n_points);
  if (use == 0 || dlin.empty() || dth.empty()) return NDT2D_OK;   // (the loops do not run: no candidate, best = 0)
  if (m->wide == nullptr)
  {
    const int rc = ndt2d_wide_create(m->dev, kWideMaxTiles, &m->wide);
    if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_wide_create");
  }
  if (tile_steps != 0)
  {
    uint32_t pixels = 0;
    (void)ndt2d_wide_tile(m->wide, nullptr, &pixels);
    const int rc = ndt2d_wide_set_tile(m->wide, tile_steps, pixels);
    if (rc != NDT2D_OK) return mfail(m, rc, std::string("match_wide: ") + ndt2d_wide_last_error(m->wide));
  }
  // the image of the last call is of this NDT when the matcher has not built or dropped one since
  const int reuse = m->wide_installs == m->ndt.installs() ? 1 : 0;
  m->wide_installs = ~0ull;
  double record[2] = {0.0, -1.0};
  const int rc = ndt2d_wide_match(m->wide, scan_pose_xyt, m->beams.host.data(), use, dth.data(), dth.size(), dlin.data(),
                                  dlin.size(), reuse, record, stats_out, nullptr, nullptr);
  if (rc != NDT2D_OK) return mfail(m, rc, std::string("match_wide: ") + ndt2d_wide_last_error(m->wide));
  m->wide_installs = m->ndt.installs();
  m->last_multi = false;
  if (record[1] >= 0.0)
  {
    const uint64_t best = static_cast<uint64_t>(record[1]);   // (truncates a near-tie mark, index + 0.5)
    const uint64_t n_lin = dlin.size(), per_th = n_lin * n_lin;
    if (best_index_out != nullptr) *best_index_out = best;
    if (near_tie_out != nullptr) *near_tie_out = marked_winner(record) ? 1 : 0;
    if (pose_out != nullptr)
    {
      // :128-134: the accumulated offsets of the winning candidate
      pose_out[0] = dlin[(best % per_th) / n_lin];
      pose_out[1] = dlin[best % n_lin];
      pose_out[2] = dth[best / per_th];
    }
  }
  *score_out = record[0] / use;   // :148
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

ndt2d_wide * ndt2d_matcher_wide(ndt2d_matcher * m) { return m != nullptr ? m->wide : nullptr; }

// Jobs the batched scan tracking launches at a time: the object's limit (a fleet is tens, a
// replayed bag or a graph's scans hundreds to a few thousand).
static constexpr size_t kScansSlots = 4096;

int ndt2d_matcher_match_scans(ndt2d_matcher * m, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                              const double * points_xy, const size_t * point_offsets, size_t n_scans, double * poses_out,
                              double * covariances_out, double * scores_out, uint64_t * best_index_out,
                              double * all_scores, size_t all_scores_cap, size_t * n_lattice_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_lattice_out != nullptr) *n_lattice_out = 0;
  if (n_jobs == 0) return NDT2D_OK;
  if (jobs_xyt == nullptr || scores_out == nullptr || point_offsets == nullptr)
  {
    return mfail(m, NDT2D_ERR_INVALID, "match_scans: null input");
  }
  // (the list's size is refused before the `if (!ndt_)` return, everything else of it after)
  std::string refusal = job_list_size_refusal("match_scans", n_jobs, n_scans);
  if (!refusal.empty()) return mfail(m, NDT2D_ERR_INVALID, refusal);
  if (!m->ndt.have())
  {
    fill_no_ndt(n_jobs, scores_out, best_index_out);
    return NDT2D_OK;
  }
  refusal = job_list_refusal("match_scans", jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans);
  if (!refusal.empty()) return mfail(m, NDT2D_ERR_INVALID, refusal);
  const size_t n_th = m->search.dth.size(), n_lin = m->search.dlin.size();
  const size_t n_lattice = n_th * n_lin * n_lin;
  if (n_lattice_out != nullptr) *n_lattice_out = n_lattice;
  discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
  if (m->scans == nullptr)
  {
    const int rc = ndt2d_scans_create(m->dev, kScansSlots, &m->scans);
    if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_scans_create");
  }
  double * scores_ptr = scores_if_they_fit(all_scores, all_scores_cap, n_jobs, n_lattice);
  const auto scan_of = [&](size_t k) { return job_scan != nullptr ? static_cast<size_t>(job_scan[k]) : k; };

  // the jobs of the batched call, laser_max_beams as it is (0: no beams); a job outside it -- no
  // points, or no lattice: then nothing is collected -- goes through the sequential call
  JobBatch batch;
  if (n_lattice > 0) collect_job_batch(m->laser_max_beams, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans, batch);
  m->search.ready = false;   // no search is prepared on the context
  std::vector<char> sequential(n_jobs, 1);
  const size_t n_batch = batch.size();
  m->scans_records.assign(n_jobs * kRec, 0.0);   // the batch's records in front, then moved to their jobs' slots
  double * records = m->scans_records.data();
  if (n_batch > 0)
  {
    // (all jobs in the batch: its scores are the caller's rows; else they are dealt out below)
    std::vector<double> batch_scores;
    double * batch_scores_ptr = scores_ptr;
    if (n_batch != n_jobs && scores_ptr != nullptr)
    {
      batch_scores.resize(n_batch * n_lattice);
      batch_scores_ptr = batch_scores.data();
    }
    const int rc = ndt2d_scans_match(m->scans, batch.xyt.data(), batch.scan.data(), n_batch, batch.beams.data(),
                                     batch.beam_offsets.data(), batch.scans(), m->search.dth.data(), n_th, m->search.dlin.data(),
                                     n_lin, records, batch_scores_ptr);
    if (rc != NDT2D_OK) return mfail(m, rc, std::string("match_scans: ") + ndt2d_scans_last_error(m->scans));
    m->last_multi = false;
    move_match_records(batch, kRec, records);
    for (size_t j = 0; j < n_batch; ++j) sequential[batch.job[j]] = marked_winner(records + batch.job[j] * kRec);
    if (!batch_scores.empty()) deal_lattice_scores(batch, batch_scores.data(), n_lattice, sequential, scores_ptr);
  }
  const BatchOut out = {poses_out, covariances_out, scores_out, best_index_out, scores_ptr, n_lattice};
  return finish_slots(
    m, n_jobs, records, sequential, out, "match_scans: job ",
    [&](size_t k, const SlotOut & o) {
      const size_t sc = scan_of(k);
      return match_alone(m, jobs_xyt + 3 * k, points_xy + 2 * point_offsets[sc], point_offsets[sc + 1] - point_offsets[sc], o,
                         n_lattice);
    },
    [&](size_t k) {
      // the N of `best / N` (:148) is the job's own scan's
      m->search.n_use = batch.scan_beams(batch.sent[scan_of(k)]);
      m->search.ready = false;   // (a sequential call in between prepared a search of its own)
    });
  NDT2D_C_CATCH(m)
}

ndt2d_scans * ndt2d_matcher_scans(ndt2d_matcher * m) { return m != nullptr ? m->scans : nullptr; }

// Jobs the Newton registration launches at a time: the object's limit, as match_scans.
static constexpr size_t kRefineSlots = 4096;

int ndt2d_matcher_refine_scans(ndt2d_matcher * m, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                               const double * points_xy, const size_t * point_offsets, size_t n_scans, uint32_t max_evals,
                               double tol_lin, double tol_ang, double * poses_out, double * scores_out,
                               double * start_scores_out, double * gradients_out, double * hessians_out,
                               int32_t * status_out, uint32_t * evals_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  if (jobs_xyt == nullptr || poses_out == nullptr || scores_out == nullptr || status_out == nullptr || point_offsets == nullptr)
  {
    return mfail(m, NDT2D_ERR_INVALID, "refine_scans: null input");
  }
  const RefineRules rules = {max_evals, tol_lin, tol_ang};
  int rc = check_job_input(m, "refine_scans", jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans, &rules);
  if (rc != NDT2D_OK) return rc;
  const RefineOut out = {poses_out, scores_out, start_scores_out, gradients_out, hessians_out, status_out, evals_out};
  fill_no_overlap(jobs_xyt, n_jobs, out);
  if (!m->ndt.have()) return NDT2D_OK;
  discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
  if (m->refine == nullptr)
  {
    rc = ndt2d_refine_create(m->dev, kRefineSlots, &m->refine);
    if (rc != NDT2D_OK) return dev_fail(m, rc, "ndt2d_refine_create");
  }
  if (ndt2d_refine_set_neighbourhood(m->refine, m->refine_cells) != NDT2D_OK)
  {
    return mfail(m, NDT2D_ERR_INTERNAL, std::string("refine_scans: ") + ndt2d_refine_last_error(m->refine));
  }
  JobBatch batch;
  collect_job_batch(m->laser_max_beams != 0 ? m->laser_max_beams : kEveryPoint, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets,
                    n_scans, batch);
  if (batch.size() == 0) return NDT2D_OK;
  m->refine_records.assign(batch.size() * NDT2D_REFINE_RECORD_DOUBLES, 0.0);
  rc = ndt2d_refine_run(m->refine, batch.xyt.data(), batch.scan.data(), batch.size(), batch.beams.data(), batch.beam_offsets.data(),
                        batch.scans(), max_evals, tol_lin, tol_ang, m->refine_records.data());
  if (rc != NDT2D_OK) return mfail(m, rc, std::string("refine_scans: ") + ndt2d_refine_last_error(m->refine));
  deal_refine_records(batch, m->refine_records.data(), NDT2D_REFINE_RECORD_DOUBLES, out);
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

ndt2d_refine * ndt2d_matcher_refine(ndt2d_matcher * m) { return m != nullptr ? m->refine : nullptr; }

int ndt2d_matcher_set_refine_neighbourhood(ndt2d_matcher * m, uint32_t cells)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (cells != 1 && cells != 9)
  {
    return mfail(m, NDT2D_ERR_INVALID, "set_refine_neighbourhood: " + std::to_string(cells) + " cells (1 or 9)");
  }
  m->refine_cells = cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_refine_neighbourhood(ndt2d_matcher * m, uint32_t * out)
{
  NDT2D_C_TRY
  if (m == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = m->refine_cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

// Jobs the match verification launches at a time: the object's limit, as refine_scans.
static constexpr size_t kVerifySlots = 4096;

int ndt2d_matcher_verify_scans(ndt2d_matcher * m, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                               const double * points_xy, const size_t * point_offsets, size_t n_scans, size_t max_beams,
                               uint32_t * records_out, size_t * beam_offsets_out, uint8_t * beam_class_out,
                               double * beam_m2_out, uint32_t * beam_cells_out, size_t beam_cap)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0)
  {
    if (beam_offsets_out != nullptr) beam_offsets_out[0] = 0;
    return NDT2D_OK;
  }
  if (jobs_xyt == nullptr || records_out == nullptr || point_offsets == nullptr)
  {
    return mfail(m, NDT2D_ERR_INVALID, "verify_scans: null input");
  }
  int rc = check_job_input(m, "verify_scans", jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans, nullptr);
  if (rc != NDT2D_OK) return rc;
  if (!m->ndt.have()) return mfail(m, NDT2D_ERR_NO_GRID, "verify_scans: no NDT in place");
  JobBatch batch;
  collect_job_batch(max_beams != 0 ? max_beams : kEveryPoint, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans, batch);
  const VerifyOut out = {records_out, beam_offsets_out, beam_class_out, beam_m2_out, beam_cells_out, beam_cap};
  return verify_batch(m, "verify_scans", batch, n_jobs, out, true, [&](uint32_t * records) {
    discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
    if (m->verify == nullptr)
    {
      const int crc = ndt2d_verify_create(m->dev, kVerifySlots, &m->verify);
      if (crc != NDT2D_OK) return dev_fail(m, crc, "ndt2d_verify_create");
    }
    if (ndt2d_verify_set_neighbourhood(m->verify, m->verify_cells) != NDT2D_OK ||
        ndt2d_verify_set_gates(m->verify, m->verify_gate_inlier, m->verify_gate_pierce) != NDT2D_OK ||
        ndt2d_verify_set_rays(m->verify, m->verify_rays ? 1 : 0) != NDT2D_OK)
    {
      return mfail(m, NDT2D_ERR_INTERNAL, std::string("verify_scans: ") + ndt2d_verify_last_error(m->verify));
    }
    const int vrc = ndt2d_verify_run(m->verify, batch.xyt.data(), batch.scan.data(), batch.size(), batch.beams.data(),
                                     batch.beam_offsets.data(), batch.scans(), records, beam_class_out, beam_m2_out, beam_cells_out);
    return vrc == NDT2D_OK ? NDT2D_OK : mfail(m, vrc, std::string("verify_scans: ") + ndt2d_verify_last_error(m->verify));
  });
  NDT2D_C_CATCH(m)
}

ndt2d_verify * ndt2d_matcher_verify(ndt2d_matcher * m) { return m != nullptr ? m->verify : nullptr; }

int ndt2d_matcher_set_verify_neighbourhood(ndt2d_matcher * m, uint32_t cells)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (cells != 1 && cells != 9)
  {
    return mfail(m, NDT2D_ERR_INVALID, "set_verify_neighbourhood: " + std::to_string(cells) + " cells (1 or 9)");
  }
  m->verify_cells = cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_verify_neighbourhood(ndt2d_matcher * m, uint32_t * out)
{
  NDT2D_C_TRY
  if (m == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = m->verify_cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_verify_gates(ndt2d_matcher * m, double gate_inlier, double gate_pierce)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (!(gate_inlier >= 0.0) || !(gate_pierce >= 0.0) || !std::isfinite(gate_inlier) || !std::isfinite(gate_pierce))
  {
    return mfail(m, NDT2D_ERR_INVALID, "set_verify_gates: a gate is negative or not finite");
  }
  m->verify_gate_inlier = gate_inlier;
  m->verify_gate_pierce = gate_pierce;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_verify_gates(ndt2d_matcher * m, double * gate_inlier_out, double * gate_pierce_out)
{
  NDT2D_C_TRY
  if (m == nullptr || gate_inlier_out == nullptr || gate_pierce_out == nullptr) return NDT2D_ERR_INVALID;
  *gate_inlier_out = m->verify_gate_inlier;
  *gate_pierce_out = m->verify_gate_pierce;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_set_verify_rays(ndt2d_matcher * m, int enabled)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (enabled != 0 && enabled != 1) return mfail(m, NDT2D_ERR_INVALID, "set_verify_rays: " + std::to_string(enabled) + " (0 or 1)");
  m->verify_rays = enabled != 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_verify_rays(ndt2d_matcher * m, int * out)
{
  NDT2D_C_TRY
  if (m == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = m->verify_rays ? 1 : 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_refine_candidates(ndt2d_matcher * m, const size_t * cand_offsets, const size_t * ids,
                                    const double * poses_xyt, size_t n_candidates, const double * jobs_xyt,
                                    const uint32_t * job_scan, const uint32_t * job_candidate, size_t n_jobs,
                                    const double * points_xy, const size_t * point_offsets, size_t n_scans,
                                    uint32_t max_evals, double tol_lin, double tol_ang, double * poses_out,
                                    double * scores_out, double * start_scores_out, double * gradients_out,
                                    double * hessians_out, int32_t * status_out, uint32_t * evals_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  if (jobs_xyt == nullptr || poses_out == nullptr || scores_out == nullptr || status_out == nullptr || point_offsets == nullptr ||
      cand_offsets == nullptr || ids == nullptr || poses_xyt == nullptr)
  {
    return mfail(m, NDT2D_ERR_INVALID, "refine_candidates: null input");
  }
  if (n_candidates == 0 || n_candidates > (1u << 20)) return mfail(m, NDT2D_ERR_INVALID, "refine_candidates: no candidates, or too many");
  const RefineRules rules = {max_evals, tol_lin, tol_ang};
  int rc = check_job_input(m, "refine_candidates", jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans, &rules);
  if (rc != NDT2D_OK) return rc;
  rc = check_job_candidates(m, "refine_candidates", job_candidate, n_jobs, n_candidates);
  if (rc != NDT2D_OK) return rc;
  const RefineOut out = {poses_out, scores_out, start_scores_out, gradients_out, hessians_out, status_out, evals_out};
  discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
  rc = ensure_closure(m);
  if (rc != NDT2D_OK) return rc;
  if (ndt2d_closure_set_neighbourhood(m->closure, m->refine_cells) != NDT2D_OK)
  {
    return mfail(m, NDT2D_ERR_INTERNAL, std::string("refine_candidates: ") + ndt2d_closure_last_error(m->closure));
  }
  JobBatch batch;
  collect_job_batch(m->laser_max_beams != 0 ? m->laser_max_beams : kEveryPoint, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets,
                    n_scans, batch);
  if (batch.size() == 0)
  {
    fill_no_overlap(jobs_xyt, n_jobs, out);
    return NDT2D_OK;
  }
  const std::vector<uint32_t> batch_candidate = batch_candidates(batch, job_candidate);
  rc = ndt2d_scanstore_set_eigenvalue_form(m->stores[0], eigen_form_name(m));
  m->refine_records.assign(batch.size() * NDT2D_REFINE_RECORD_DOUBLES, 0.0);
  if (rc == NDT2D_OK)
  {
    rc = ndt2d_closure_refine(m->closure, n_candidates, cand_offsets, ids, poses_xyt, m->resolution, m->range_max, batch.xyt.data(),
                              batch.scan.data(), batch_candidate.data(), batch.size(), batch.beams.data(), batch.beam_offsets.data(),
                              batch.scans(), max_evals, tol_lin, tol_ang, m->refine_records.data());
  }
  // (a refused call -- a candidate the closure does not take -- leaves the outputs as they were)
  if (rc != NDT2D_OK) return mfail(m, rc, std::string("refine_candidates: ") + ndt2d_closure_last_error(m->closure));
  fill_no_overlap(jobs_xyt, n_jobs, out);   // (the jobs of a scan without points keep this)
  deal_refine_records(batch, m->refine_records.data(), NDT2D_REFINE_RECORD_DOUBLES, out);
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_matcher_verify_candidates(ndt2d_matcher * m, const size_t * cand_offsets, const size_t * ids,
                                    const double * poses_xyt, size_t n_candidates, const double * jobs_xyt,
                                    const uint32_t * job_scan, const uint32_t * job_candidate, size_t n_jobs,
                                    const double * points_xy, const size_t * point_offsets, size_t n_scans, size_t max_beams,
                                    uint32_t * records_out, size_t * beam_offsets_out, uint8_t * beam_class_out,
                                    double * beam_m2_out, uint32_t * beam_cells_out, size_t beam_cap)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0)
  {
    if (beam_offsets_out != nullptr) beam_offsets_out[0] = 0;
    return NDT2D_OK;
  }
  if (jobs_xyt == nullptr || records_out == nullptr || point_offsets == nullptr || cand_offsets == nullptr || ids == nullptr ||
      poses_xyt == nullptr)
  {
    return mfail(m, NDT2D_ERR_INVALID, "verify_candidates: null input");
  }
  if (n_candidates == 0 || n_candidates > (1u << 20)) return mfail(m, NDT2D_ERR_INVALID, "verify_candidates: no candidates, or too many");
  int rc = check_job_input(m, "verify_candidates", jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans, nullptr);
  if (rc != NDT2D_OK) return rc;
  rc = check_job_candidates(m, "verify_candidates", job_candidate, n_jobs, n_candidates);
  if (rc != NDT2D_OK) return rc;
  JobBatch batch;
  collect_job_batch(max_beams != 0 ? max_beams : kEveryPoint, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans, batch);
  const VerifyOut out = {records_out, beam_offsets_out, beam_class_out, beam_m2_out, beam_cells_out, beam_cap};
  // (a refused call -- a candidate the closure does not take -- leaves the outputs as they were)
  return verify_batch(m, "verify_candidates", batch, n_jobs, out, false, [&](uint32_t * records) {
    discard_ahead(m);   // a search launched ahead by scoreScan is waited out and dropped
    int crc = ensure_closure(m);
    if (crc != NDT2D_OK) return crc;
    if (ndt2d_closure_set_verify_neighbourhood(m->closure, m->verify_cells) != NDT2D_OK ||
        ndt2d_closure_set_verify_gates(m->closure, m->verify_gate_inlier, m->verify_gate_pierce) != NDT2D_OK ||
        ndt2d_closure_set_verify_rays(m->closure, m->verify_rays ? 1 : 0) != NDT2D_OK)
    {
      return mfail(m, NDT2D_ERR_INTERNAL, std::string("verify_candidates: ") + ndt2d_closure_last_error(m->closure));
    }
    const std::vector<uint32_t> batch_candidate = batch_candidates(batch, job_candidate);
    crc = ndt2d_scanstore_set_eigenvalue_form(m->stores[0], eigen_form_name(m));
    if (crc == NDT2D_OK)
    {
      crc = ndt2d_closure_verify(m->closure, n_candidates, cand_offsets, ids, poses_xyt, m->resolution, m->range_max, batch.xyt.data(),
                                 batch.scan.data(), batch_candidate.data(), batch.size(), batch.beams.data(), batch.beam_offsets.data(),
                                 batch.scans(), records, beam_class_out, beam_m2_out, beam_cells_out);
    }
    return crc == NDT2D_OK ? NDT2D_OK : mfail(m, crc, std::string("verify_candidates: ") + ndt2d_closure_last_error(m->closure));
  });
  NDT2D_C_CATCH(m)
}

}  // extern "C"
