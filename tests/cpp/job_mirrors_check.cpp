// The five matcher mirrors of ndt_2d_amd/plugin (track_scans_hip.hpp, refine_hip.hpp,
// verify_hip.hpp, relocalize_hip.hpp, loop_closure_hip.hpp) run on stand-ins for the
// ndt2d_matcher_* entry points: every stand-in records the arrays it is given by value and writes
// canned outputs; the expected values are written out by hand.  A program of its own, built with
// the host compiler and the sanitizers, run directly (tests/test_job_list_host.py).  Prints OK, or
// FAILED lines.
//
// The one list: 5 jobs over 4 scans of 6, 0, 3 and 9 points, limit 4; jobs 0 and 3 share scan 0,
// scan 1 is empty, scan 2 is shorter than the limit, scan 3 longer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "loop_closure_hip.hpp"
#include "refine_hip.hpp"
#include "relocalize_hip.hpp"
#include "track_scans_hip.hpp"
#include "verify_hip.hpp"

#include "ndt2d_refine_step.h"

static int failures = 0;

#define CHECK(cond)                                                      \
  do                                                                     \
  {                                                                      \
    if (!(cond))                                                         \
    {                                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

struct ndt2d_matcher
{
  int unused;
};
struct ndt2d_scans
{
  int unused;
};
struct ndt2d_starts
{
  int unused;
};
struct ndt2d_refine
{
  int unused;
};
struct ndt2d_verify
{
  int unused;
};

namespace
{

using VecD = std::vector<double>;
using VecZ = std::vector<std::size_t>;
using VecU = std::vector<std::uint32_t>;

// What a stand-in was given, by value.
struct Call
{
  std::string name;
  VecD jobs, points, cand_poses;
  VecU job_scan, job_candidate;
  VecZ offsets, cand_offsets, ids;
  std::size_t n_jobs = 0, n_scans = 0, n_candidates = 0, max_beams = 0, cap = 0;
  std::uint32_t max_evals = 0;
  double tol_lin = 0.0, tol_ang = 0.0;
  bool has_job_scan = false, has_job_candidate = false, has_gradients = false, has_table = false;
  bool has_classes = false, has_m2 = false, has_cells = false, has_best = false, has_all_scores = false;
  std::size_t all_scores_cap = 0;
};

std::vector<Call> calls;
bool fail_next = false;                 // the next stand-in that may fail refuses
std::vector<VecD> candidate_scores;     // per ndt2d_matcher_match_candidates call
VecU settings;                          // what the setters were given, in order
std::size_t stored = 0;

ndt2d_matcher the_matcher{0};
ndt2d_scans the_scans{0};
ndt2d_starts the_starts{0};
ndt2d_refine the_refine{0};
ndt2d_verify the_verify{0};

int refused()
{
  if (!fail_next) return NDT2D_OK;
  fail_next = false;
  return NDT2D_ERR_INVALID;
}

void take_list(Call & c, const double * jobs_xyt, const std::uint32_t * job_scan, std::size_t n_jobs, const double * points_xy,
               const std::size_t * point_offsets, std::size_t n_scans)
{
  c.n_jobs = n_jobs;
  c.n_scans = n_scans;
  c.jobs.assign(jobs_xyt, jobs_xyt + 3 * n_jobs);
  c.has_job_scan = job_scan != nullptr;
  if (job_scan != nullptr) c.job_scan.assign(job_scan, job_scan + n_jobs);
  c.offsets.assign(point_offsets, point_offsets + n_scans + 1);
  c.points.assign(points_xy, points_xy + 2 * point_offsets[n_scans]);
}

void take_candidates(Call & c, const std::size_t * cand_offsets, const std::size_t * ids, const double * poses_xyt, std::size_t n)
{
  c.n_candidates = n;
  c.cand_offsets.assign(cand_offsets, cand_offsets + n + 1);
  c.ids.assign(ids, ids + cand_offsets[n]);
  c.cand_poses.assign(poses_xyt, poses_xyt + 3 * cand_offsets[n]);
}

// job k's correction: (0.5, -0.25, 0.125) x (k + 1); its covariance: 9 k + d; its score: -(k + 1) / 8
void write_matches(std::size_t n, double * poses_out, double * covariances_out, double * scores_out)
{
  for (std::size_t k = 0; k < n; ++k)
  {
    const double f = static_cast<double>(k + 1);
    poses_out[3 * k] = 0.5 * f;
    poses_out[3 * k + 1] = -0.25 * f;
    poses_out[3 * k + 2] = 0.125 * f;
    for (int d = 0; d < 9; ++d) covariances_out[9 * k + d] = static_cast<double>(9 * k) + d;
    scores_out[k] = -f / 8.0;
  }
}

// job k's refined pose: its own + 1/16 each; score -0.6 from -0.5; gradient k + d / 2; Hessian
// [[2, 1, 0], [1, 4, 0], [0, 0, 8]]; evals {3 + k, 2 + k}.  `dead`: the job that did not run.
void write_refined(const double * jobs_xyt, std::size_t n, std::size_t dead, std::size_t stalled, double * poses_out,
                   double * scores_out, double * start_scores_out, double * gradients_out, double * hessians_out,
                   std::int32_t * status_out, std::uint32_t * evals_out)
{
  const double H[9] = {2.0, 1.0, 0.0, 1.0, 4.0, 0.0, 0.0, 0.0, 8.0};
  for (std::size_t k = 0; k < n; ++k)
  {
    for (int d = 0; d < 3; ++d)
    {
      poses_out[3 * k + d] = jobs_xyt[3 * k + d] + 0.0625;
      if (gradients_out != nullptr) gradients_out[3 * k + d] = static_cast<double>(k) + 0.5 * d;
    }
    scores_out[k] = -0.6;
    start_scores_out[k] = -0.5;
    for (int d = 0; d < 9; ++d) hessians_out[9 * k + d] = H[d];
    status_out[k] = k == dead ? NDT2D_REFINE_NO_OVERLAP : k == stalled ? NDT2D_REFINE_STALLED : NDT2D_REFINE_CONVERGED;
    evals_out[2 * k] = k == dead ? 0u : static_cast<std::uint32_t>(3 + k);
    evals_out[2 * k + 1] = k == dead ? 0u : static_cast<std::uint32_t>(2 + k);
  }
}

}  // namespace

extern "C" {

const char * ndt2d_matcher_last_error(ndt2d_matcher *) { return "canned refusal"; }

ndt2d_scans * ndt2d_matcher_scans(ndt2d_matcher *) { return &the_scans; }
ndt2d_starts * ndt2d_matcher_starts(ndt2d_matcher *) { return &the_starts; }
ndt2d_refine * ndt2d_matcher_refine(ndt2d_matcher *) { return &the_refine; }
ndt2d_verify * ndt2d_matcher_verify(ndt2d_matcher *) { return &the_verify; }

int ndt2d_scans_last_ms(ndt2d_scans *, float * a, float * b)
{
  *a = 1.5f;
  *b = 2.5f;
  return NDT2D_OK;
}
int ndt2d_starts_last_ms(ndt2d_starts *, float * a, float * b)
{
  *a = 3.5f;
  *b = 4.5f;
  return NDT2D_OK;
}
int ndt2d_refine_last_ms(ndt2d_refine *, float * a, float * b)
{
  *a = 5.5f;
  *b = 6.5f;
  return NDT2D_OK;
}
int ndt2d_verify_last_ms(ndt2d_verify *, float * a, float * b)
{
  *a = 7.5f;
  *b = 8.5f;
  return NDT2D_OK;
}

int ndt2d_refine_covariance(const double * H6, double * cov9_out)
{
  const double H[6] = {H6[0], H6[1], H6[2], H6[3], H6[4], H6[5]};
  double cov[9];
  if (!ndt2d::refine::covariance(H, cov)) return NDT2D_ERR_STATE;
  for (int d = 0; d < 9; ++d) cov9_out[d] = cov[d];
  return NDT2D_OK;
}

int ndt2d_matcher_set_refine_neighbourhood(ndt2d_matcher *, std::uint32_t cells)
{
  settings.push_back(cells);
  return refused();
}
int ndt2d_matcher_refine_neighbourhood(ndt2d_matcher *, std::uint32_t * out)
{
  *out = 9u;
  return refused();
}
int ndt2d_matcher_set_verify_neighbourhood(ndt2d_matcher *, std::uint32_t cells)
{
  settings.push_back(100u + cells);
  return refused();
}
int ndt2d_matcher_set_verify_gates(ndt2d_matcher *, double gate_inlier, double gate_pierce)
{
  settings.push_back(static_cast<std::uint32_t>(1000.0 * gate_inlier + gate_pierce));
  return refused();
}
int ndt2d_matcher_set_verify_rays(ndt2d_matcher *, int enabled)
{
  settings.push_back(200u + static_cast<std::uint32_t>(enabled));
  return refused();
}

int ndt2d_matcher_store_scan(ndt2d_matcher *, const double *, std::size_t, std::size_t * id_out)
{
  if (refused() != NDT2D_OK) return NDT2D_ERR_INVALID;
  *id_out = stored++;
  return NDT2D_OK;
}
int ndt2d_matcher_drop_scans(ndt2d_matcher *)
{
  stored = 0;
  return refused();
}

int ndt2d_matcher_match_scans(ndt2d_matcher *, const double * jobs_xyt, const std::uint32_t * job_scan, std::size_t n_jobs,
                              const double * points_xy, const std::size_t * point_offsets, std::size_t n_scans, double * poses_out,
                              double * covariances_out, double * scores_out, std::uint64_t * best_index_out, double * all_scores,
                              std::size_t all_scores_cap, std::size_t * n_lattice_out)
{
  Call c;
  c.name = "match_scans";
  take_list(c, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans);
  c.has_best = best_index_out != nullptr;
  c.has_all_scores = all_scores != nullptr || n_lattice_out != nullptr;
  c.all_scores_cap = all_scores_cap;
  calls.push_back(c);
  if (refused() != NDT2D_OK) return NDT2D_ERR_INVALID;
  write_matches(n_jobs, poses_out, covariances_out, scores_out);
  for (std::size_t k = 0; k < n_jobs; ++k) best_index_out[k] = k == 1 ? NDT2D_NO_INDEX : 100u + k;
  return NDT2D_OK;
}

int ndt2d_matcher_match_starts(ndt2d_matcher *, const double * starts_xyt, std::size_t n_starts, const double * points_xy,
                               std::size_t n_points, double * poses_out, double * covariances_out, double * scores_out,
                               std::uint64_t * best_index_out, double * all_scores, std::size_t all_scores_cap,
                               std::size_t * n_lattice_out)
{
  Call c;
  c.name = "match_starts";
  c.n_jobs = n_starts;
  c.jobs.assign(starts_xyt, starts_xyt + 3 * n_starts);
  c.points.assign(points_xy, points_xy + 2 * n_points);
  c.has_best = best_index_out != nullptr;
  c.has_all_scores = all_scores != nullptr || n_lattice_out != nullptr;
  c.all_scores_cap = all_scores_cap;
  calls.push_back(c);
  if (refused() != NDT2D_OK) return NDT2D_ERR_STATE;
  write_matches(n_starts, poses_out, covariances_out, scores_out);
  const double scores[4] = {-0.25, -0.75, -0.5, -0.875};
  for (std::size_t k = 0; k < n_starts; ++k)
  {
    scores_out[k] = scores[k % 4];
    best_index_out[k] = k == 3 ? NDT2D_NO_INDEX : 7u;
  }
  return NDT2D_OK;
}

int ndt2d_matcher_refine_scans(ndt2d_matcher *, const double * jobs_xyt, const std::uint32_t * job_scan, std::size_t n_jobs,
                               const double * points_xy, const std::size_t * point_offsets, std::size_t n_scans,
                               std::uint32_t max_evals, double tol_lin, double tol_ang, double * poses_out, double * scores_out,
                               double * start_scores_out, double * gradients_out, double * hessians_out, std::int32_t * status_out,
                               std::uint32_t * evals_out)
{
  Call c;
  c.name = "refine_scans";
  take_list(c, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans);
  c.max_evals = max_evals;
  c.tol_lin = tol_lin;
  c.tol_ang = tol_ang;
  c.has_gradients = gradients_out != nullptr;
  calls.push_back(c);
  if (refused() != NDT2D_OK) return NDT2D_ERR_INVALID;
  write_refined(jobs_xyt, n_jobs, 1, n_jobs, poses_out, scores_out, start_scores_out, gradients_out, hessians_out, status_out,
                evals_out);
  return NDT2D_OK;
}

// Records {beams, k, k + 1, k + 2, k + 3, k + 4, k + 5, 0} with beams = min(max_beams or all, the
// scan's points); the table from them; beam i of the call: class i + 1, m2 i / 2, cells 100 + i, 200 + i.
int verify_stand_in(Call & c, std::size_t max_beams, std::uint32_t * records_out, std::size_t * beam_offsets_out,
                    std::uint8_t * beam_class_out, double * beam_m2_out, std::uint32_t * beam_cells_out, std::size_t beam_cap)
{
  c.max_beams = max_beams;
  c.cap = beam_cap;
  c.has_table = beam_offsets_out != nullptr;
  c.has_classes = beam_class_out != nullptr;
  c.has_m2 = beam_m2_out != nullptr;
  c.has_cells = beam_cells_out != nullptr;
  calls.push_back(c);
  if (refused() != NDT2D_OK) return NDT2D_ERR_NO_GRID;
  std::size_t at = 0;
  for (std::size_t k = 0; k < c.n_jobs; ++k)
  {
    const std::size_t sc = c.has_job_scan ? c.job_scan[k] : k;
    const std::size_t points = c.offsets[sc + 1] - c.offsets[sc];
    const std::size_t beams = max_beams == 0 || points < max_beams ? points : max_beams;
    std::uint32_t * rec = records_out + NDT2D_VERIFY_RECORD_U32 * k;
    rec[0] = static_cast<std::uint32_t>(beams);
    for (std::uint32_t d = 1; d < 7; ++d) rec[d] = static_cast<std::uint32_t>(k) + d - 1u;
    rec[7] = 0u;
    if (beam_offsets_out != nullptr) beam_offsets_out[k] = at;
    at += beams;
  }
  if (beam_offsets_out != nullptr) beam_offsets_out[c.n_jobs] = at;
  for (std::size_t i = 0; i < at && i < beam_cap; ++i)
  {
    if (beam_class_out != nullptr) beam_class_out[i] = static_cast<std::uint8_t>(i + 1);
    if (beam_m2_out != nullptr) beam_m2_out[i] = 0.5 * static_cast<double>(i);
    if (beam_cells_out != nullptr)
    {
      beam_cells_out[2 * i] = 100u + static_cast<std::uint32_t>(i);
      beam_cells_out[2 * i + 1] = 200u + static_cast<std::uint32_t>(i);
    }
  }
  return NDT2D_OK;
}

int ndt2d_matcher_verify_scans(ndt2d_matcher *, const double * jobs_xyt, const std::uint32_t * job_scan, std::size_t n_jobs,
                               const double * points_xy, const std::size_t * point_offsets, std::size_t n_scans,
                               std::size_t max_beams, std::uint32_t * records_out, std::size_t * beam_offsets_out,
                               std::uint8_t * beam_class_out, double * beam_m2_out, std::uint32_t * beam_cells_out,
                               std::size_t beam_cap)
{
  Call c;
  c.name = "verify_scans";
  take_list(c, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans);
  return verify_stand_in(c, max_beams, records_out, beam_offsets_out, beam_class_out, beam_m2_out, beam_cells_out, beam_cap);
}

int ndt2d_matcher_match_candidates(ndt2d_matcher *, const double * scan_pose_xyt, const double * points_xy, std::size_t n_points,
                                   const std::size_t * cand_offsets, const std::size_t * ids, const double * poses_xyt,
                                   std::size_t n_candidates, double * poses_out, double * covariances_out, double * scores_out,
                                   std::uint64_t * best_index_out, double * all_scores, std::size_t all_scores_cap,
                                   std::size_t * n_lattice_out)
{
  Call c;
  c.name = "match_candidates";
  c.jobs.assign(scan_pose_xyt, scan_pose_xyt + 3);
  c.points.assign(points_xy, points_xy + 2 * n_points);
  take_candidates(c, cand_offsets, ids, poses_xyt, n_candidates);
  c.has_best = best_index_out != nullptr;
  c.has_all_scores = all_scores != nullptr || n_lattice_out != nullptr;
  c.all_scores_cap = all_scores_cap;
  calls.push_back(c);
  if (refused() != NDT2D_OK) return NDT2D_ERR_HIP;
  write_matches(n_candidates, poses_out, covariances_out, scores_out);
  const VecD scores = candidate_scores.front();
  candidate_scores.erase(candidate_scores.begin());
  for (std::size_t k = 0; k < n_candidates; ++k) scores_out[k] = scores[k];
  return NDT2D_OK;
}

int ndt2d_matcher_refine_candidates(ndt2d_matcher *, const std::size_t * cand_offsets, const std::size_t * ids,
                                    const double * poses_xyt, std::size_t n_candidates, const double * jobs_xyt,
                                    const std::uint32_t * job_scan, const std::uint32_t * job_candidate, std::size_t n_jobs,
                                    const double * points_xy, const std::size_t * point_offsets, std::size_t n_scans,
                                    std::uint32_t max_evals, double tol_lin, double tol_ang, double * poses_out, double * scores_out,
                                    double * start_scores_out, double * gradients_out, double * hessians_out,
                                    std::int32_t * status_out, std::uint32_t * evals_out)
{
  Call c;
  c.name = "refine_candidates";
  take_list(c, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans);
  take_candidates(c, cand_offsets, ids, poses_xyt, n_candidates);
  c.has_job_candidate = job_candidate != nullptr;
  if (job_candidate != nullptr) c.job_candidate.assign(job_candidate, job_candidate + n_jobs);
  c.max_evals = max_evals;
  c.tol_lin = tol_lin;
  c.tol_ang = tol_ang;
  c.has_gradients = gradients_out != nullptr;
  calls.push_back(c);
  if (refused() != NDT2D_OK) return NDT2D_ERR_INVALID;
  // (job 1 stalls: its refined pose is not usable)
  write_refined(jobs_xyt, n_jobs, n_jobs, 1, poses_out, scores_out, start_scores_out, gradients_out, hessians_out, status_out,
                evals_out);
  return NDT2D_OK;
}

int ndt2d_matcher_verify_candidates(ndt2d_matcher *, const std::size_t * cand_offsets, const std::size_t * ids,
                                    const double * poses_xyt, std::size_t n_candidates, const double * jobs_xyt,
                                    const std::uint32_t * job_scan, const std::uint32_t * job_candidate, std::size_t n_jobs,
                                    const double * points_xy, const std::size_t * point_offsets, std::size_t n_scans,
                                    std::size_t max_beams, std::uint32_t * records_out, std::size_t * beam_offsets_out,
                                    std::uint8_t * beam_class_out, double * beam_m2_out, std::uint32_t * beam_cells_out,
                                    std::size_t beam_cap)
{
  Call c;
  c.name = "verify_candidates";
  take_list(c, jobs_xyt, job_scan, n_jobs, points_xy, point_offsets, n_scans);
  take_candidates(c, cand_offsets, ids, poses_xyt, n_candidates);
  c.has_job_candidate = job_candidate != nullptr;
  if (job_candidate != nullptr) c.job_candidate.assign(job_candidate, job_candidate + n_jobs);
  return verify_stand_in(c, max_beams, records_out, beam_offsets_out, beam_class_out, beam_m2_out, beam_cells_out, beam_cap);
}

}  // extern "C"

namespace
{

// The designed list.  Scan s, point i: (10 s + i, 10 s + i + 0.5).
const VecD kPoints = {0.0,  0.5,  1.0,  1.5,  2.0,  2.5,  3.0,  3.5,  4.0,  4.5,  5.0,  5.5,                       // scan 0: 6
                                                                                                                    // scan 1: 0
                      20.0, 20.5, 21.0, 21.5, 22.0, 22.5,                                                           // scan 2: 3
                      30.0, 30.5, 31.0, 31.5, 32.0, 32.5, 33.0, 33.5, 34.0, 34.5, 35.0, 35.5, 36.0, 36.5, 37.0, 37.5,
                      38.0, 38.5};                                                                                  // scan 3: 9
const VecZ kOffsets = {0, 6, 6, 9, 18};
const VecD kJobs = {1.0, 2.0, 0.25, 3.0, 4.0, 0.5, 5.0, 6.0, 0.75, 7.0, 8.0, 1.0, 9.0, 10.0, 1.25};
const VecU kJobScan = {0, 1, 2, 0, 3};
const std::size_t kScanOf[5] = {0, 1, 2, 0, 3};

bool near(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(1.0, std::fabs(b)); }

// addScan x 4 and addJob x 5, the last job through add(): the indices they return.
template <class MIRROR>
void collect(MIRROR & m)
{
  CHECK(m.jobs() == 0 && m.scans() == 0);
  CHECK(m.addScan(kPoints.data(), 6) == 0);
  CHECK(m.addScan(kPoints.data() + 12, 0) == 1);
  CHECK(m.addScan(kPoints.data() + 12, 3) == 2);
  CHECK(m.addJob(0, kJobs.data()) == 0);
  CHECK(m.addJob(1, kJobs.data() + 3) == 1);
  CHECK(m.addJob(2, kJobs.data() + 6) == 2);
  CHECK(m.addJob(0, kJobs.data() + 9) == 3);
  CHECK(m.add(kJobs.data() + 12, kPoints.data() + 18, 9) == 4);
  CHECK(m.jobs() == 5 && m.scans() == 4);
}

void check_list(const Call & c)
{
  CHECK(c.n_jobs == 5 && c.n_scans == 4);
  CHECK(c.jobs == kJobs);
  CHECK(c.has_job_scan && c.job_scan == kJobScan);
  CHECK(c.points == kPoints);
  CHECK(c.offsets == kOffsets);
}

void check_track()
{
  ndt_2d_hip::TrackScansHip t(&the_matcher);
  std::vector<ndt_2d_hip::TrackedScan> out;
  CHECK(t.track(out) && out.empty() && calls.empty());   // no job: no call
  collect(t);
  CHECK(t.track(out));
  CHECK(calls.size() == 1 && calls[0].name == "match_scans");
  check_list(calls[0]);
  CHECK(calls[0].has_best && !calls[0].has_all_scores && calls[0].all_scores_cap == 0);
  const double pose[5][3] = {{1.5, 1.75, 0.375}, {4.0, 3.5, 0.75}, {6.5, 5.25, 1.125}, {9.0, 7.0, 1.5}, {11.5, 8.75, 1.875}};
  const double correction[5][3] = {
    {0.5, -0.25, 0.125}, {1.0, -0.5, 0.25}, {1.5, -0.75, 0.375}, {2.0, -1.0, 0.5}, {2.5, -1.25, 0.625}};
  const double score[5] = {-0.125, -0.25, -0.375, -0.5, -0.625};
  CHECK(out.size() == 5);
  for (std::size_t k = 0; k < out.size(); ++k)
  {
    CHECK(out[k].job == k && out[k].scan == kScanOf[k]);
    CHECK(out[k].score == score[k] && out[k].has_winner == (k != 1));
    for (int d = 0; d < 3; ++d) CHECK(out[k].correction[d] == correction[k][d] && out[k].pose[d] == pose[k][d]);
    for (int d = 0; d < 9; ++d) CHECK(out[k].covariance[d] == static_cast<double>(9 * k) + d);
  }
  float a = 0.0f, b = 0.0f;
  CHECK(t.lastMs(&a, &b) && a == 1.5f && b == 2.5f);
  // a refusal: false, the text with the code in front; the list stays
  fail_next = true;
  CHECK(!t.track(out) && out.empty());
  CHECK(t.last_error() == "ndt2d error 1: canned refusal");
  CHECK(t.jobs() == 5 && t.scans() == 4);
  t.clear();
  CHECK(t.jobs() == 0 && t.scans() == 0);
  calls.clear();
}

void check_refine()
{
  ndt_2d_hip::RefineHip r(&the_matcher);
  std::vector<ndt_2d_hip::RefinedScan> out;
  CHECK(r.refine(out) && out.empty() && calls.empty());
  r.setRules(7, 0.5, 0.25);
  r.setLaserMaxBeams(4);
  settings.clear();
  CHECK(r.setNeighbourhood(9) && settings == VecU{9u} && r.neighbourhood() == 9u);
  collect(r);
  CHECK(r.refine(out));
  CHECK(calls.size() == 1 && calls[0].name == "refine_scans");
  check_list(calls[0]);
  CHECK(calls[0].max_evals == 7 && calls[0].tol_lin == 0.5 && calls[0].tol_ang == 0.25 && calls[0].has_gradients);
  const std::size_t beams[5] = {4, 0, 3, 4, 4};
  const double pose[5][3] = {
    {1.0625, 2.0625, 0.3125}, {3.0625, 4.0625, 0.5625}, {5.0625, 6.0625, 0.8125}, {7.0625, 8.0625, 1.0625}, {9.0625, 10.0625, 1.3125}};
  const double H[9] = {2.0, 1.0, 0.0, 1.0, 4.0, 0.0, 0.0, 0.0, 8.0};
  // the inverse of H x beams: [[4, -1], [-1, 2]] / (7 beams), 1 / (8 beams)
  const double cov4[9] = {1.0 / 7.0, -1.0 / 28.0, 0.0, -1.0 / 28.0, 1.0 / 14.0, 0.0, 0.0, 0.0, 1.0 / 32.0};
  const double cov3[9] = {4.0 / 21.0, -1.0 / 21.0, 0.0, -1.0 / 21.0, 2.0 / 21.0, 0.0, 0.0, 0.0, 1.0 / 24.0};
  CHECK(out.size() == 5);
  for (std::size_t k = 0; k < out.size(); ++k)
  {
    const ndt_2d_hip::RefinedScan & s = out[k];
    CHECK(s.job == k && s.scan == kScanOf[k] && s.beams == beams[k]);
    CHECK(s.score == -0.6 && s.start_score == -0.5);
    for (int d = 0; d < 3; ++d) CHECK(s.pose[d] == pose[k][d] && s.gradient[d] == static_cast<double>(k) + 0.5 * d);
    for (int d = 0; d < 9; ++d) CHECK(s.hessian[d] == H[d]);
    CHECK(s.evals == (k == 1 ? 0u : 3u + k) && s.steps == (k == 1 ? 0u : 2u + k));
    CHECK(s.status == (k == 1 ? NDT2D_REFINE_NO_OVERLAP : NDT2D_REFINE_CONVERGED) && s.converged() == (k != 1));
    CHECK(s.has_covariance == (k != 1));
    const double * want = beams[k] == 3 ? cov3 : cov4;
    for (int d = 0; d < 9; ++d) CHECK(k == 1 ? s.covariance[d] == 0.0 : near(s.covariance[d], want[d]));
  }
  float a = 0.0f, b = 0.0f;
  CHECK(r.lastMs(&a, &b) && a == 5.5f && b == 6.5f);
  // every point: a limit above the longest scan
  r.setLaserMaxBeams(100);
  CHECK(r.refine(out) && out.size() == 5);
  CHECK(out[0].beams == 6 && out[1].beams == 0 && out[2].beams == 3 && out[3].beams == 6 && out[4].beams == 9);
  fail_next = true;
  CHECK(!r.refine(out) && out.empty());
  CHECK(r.last_error() == "ndt2d error 1: canned refusal");
  fail_next = true;
  CHECK(!r.setNeighbourhood(5) && r.last_error() == "ndt2d error 1: canned refusal");
  r.clear();
  CHECK(r.jobs() == 0 && r.scans() == 0);
  calls.clear();
}

void check_verify()
{
  ndt_2d_hip::VerifyHip v(&the_matcher);
  std::vector<ndt_2d_hip::VerifiedScan> out;
  CHECK(v.verify(out) && out.empty() && calls.empty());
  settings.clear();
  CHECK(v.setNeighbourhood(9) && v.setGates(9.0, 1.0) && v.setRays(true));
  CHECK((settings == VecU{109u, 9001u, 201u}));
  v.setMaxBeams(4);
  collect(v);
  // counts only: no per-beam array goes out, the capacity does
  CHECK(v.verify(out));
  CHECK(calls.size() == 1 && calls[0].name == "verify_scans");
  check_list(calls[0]);
  CHECK(calls[0].max_beams == 4 && calls[0].cap == 15 && calls[0].has_table);
  CHECK(!calls[0].has_classes && !calls[0].has_m2 && !calls[0].has_cells);
  CHECK(out.size() == 5 && out[4].classes.empty() && out[4].m2.empty() && out[4].cells.empty());
  // with the beams
  v.setWantBeams(true);
  CHECK(v.verify(out));
  CHECK(calls.size() == 2);
  check_list(calls[1]);
  CHECK(calls[1].max_beams == 4 && calls[1].cap == 15 && calls[1].has_table);
  CHECK(calls[1].has_classes && calls[1].has_m2 && calls[1].has_cells);
  const std::uint32_t beams[5] = {4, 0, 3, 4, 4};
  const std::size_t first[6] = {0, 4, 4, 7, 11, 15};
  CHECK(out.size() == 5);
  for (std::size_t k = 0; k < out.size(); ++k)
  {
    const ndt_2d_hip::VerifiedScan & s = out[k];
    const std::uint32_t u = static_cast<std::uint32_t>(k);
    CHECK(s.job == k && s.scan == kScanOf[k] && s.beams == beams[k]);
    CHECK(s.off == u && s.unseen == u + 1 && s.outlier == u + 2 && s.inlier == u + 3 && s.pierced == u + 4 && s.walked == u + 5);
    CHECK(s.classes.size() == beams[k] && s.m2.size() == beams[k] && s.cells.size() == 2 * beams[k]);
    for (std::size_t i = 0; i < s.classes.size(); ++i)
    {
      const std::size_t g = first[k] + i;
      CHECK(s.classes[i] == g + 1 && s.m2[i] == 0.5 * static_cast<double>(g));
      CHECK(s.cells[2 * i] == 100 + g && s.cells[2 * i + 1] == 200 + g);
    }
  }
  // class 3 (inlier) is explained, 2 (outlier) and 3 | 4 (pierced) are not: beams 2, 1 and 6 of the call
  CHECK(out[0].explained(2) && !out[0].explained(1) && !out[2].explained(2));
  // 0: every point
  v.setMaxBeams(0);
  CHECK(v.verify(out) && calls.size() == 3 && calls[2].max_beams == 0 && calls[2].cap == 24);
  CHECK(out[0].beams == 6 && out[1].beams == 0 && out[2].beams == 3 && out[3].beams == 6 && out[4].beams == 9);
  CHECK(out[4].classes.size() == 9 && out[4].classes[0] == 16 && out[4].cells[17] == 223);
  float a = 0.0f, b = 0.0f;
  CHECK(v.lastMs(&a, &b) && a == 7.5f && b == 8.5f);
  fail_next = true;
  CHECK(!v.verify(out) && out.empty());
  CHECK(v.last_error() == "ndt2d error 2: canned refusal");
  v.clear();
  CHECK(v.jobs() == 0 && v.scans() == 0);
  calls.clear();
}

void check_relocalize()
{
  ndt_2d_hip::RelocalizeHip r(&the_matcher);
  std::vector<ndt_2d_hip::Relocalization> out;
  CHECK(r.relocalize(kJobs.data(), 0, kPoints.data(), 6, false, 0.0, out) && out.empty() && calls.empty());
  CHECK(r.relocalize(kJobs.data(), 4, kPoints.data(), 6, false, 0.0, out));
  CHECK(calls.size() == 1 && calls[0].name == "match_starts" && calls[0].n_jobs == 4);
  CHECK(calls[0].jobs == VecD(kJobs.begin(), kJobs.begin() + 12) && calls[0].points == VecD(kPoints.begin(), kPoints.begin() + 12));
  CHECK(calls[0].has_best && !calls[0].has_all_scores && calls[0].all_scores_cap == 0);
  // scores -0.25, -0.75, -0.5, -0.875 (no winner): starts 1, 2, 0, then 3
  const std::size_t order[4] = {1, 2, 0, 3};
  const double score[4] = {-0.75, -0.5, -0.25, -0.875};
  const double pose[4][3] = {{4.0, 3.5, 0.75}, {6.5, 5.25, 1.125}, {1.5, 1.75, 0.375}, {9.0, 7.0, 1.5}};
  CHECK(out.size() == 4);
  for (std::size_t i = 0; i < out.size(); ++i)
  {
    CHECK(out[i].start == order[i] && out[i].score == score[i] && out[i].has_winner == (order[i] != 3));
    for (int d = 0; d < 3; ++d) CHECK(out[i].pose[d] == pose[i][d]);
    for (int d = 0; d < 9; ++d) CHECK(out[i].covariance[d] == static_cast<double>(9 * order[i]) + d);
  }
  CHECK(r.relocalize(kJobs.data(), 4, kPoints.data(), 6, true, -0.6, out));
  CHECK(out.size() == 2 && out[0].start == 1 && out[1].start == 3);
  float a = 0.0f, b = 0.0f;
  CHECK(r.lastMs(&a, &b) && a == 3.5f && b == 4.5f);
  fail_next = true;
  CHECK(!r.relocalize(kJobs.data(), 4, kPoints.data(), 6, false, 0.0, out) && out.empty());
  CHECK(r.last_error() == "ndt2d error 5: canned refusal");
  calls.clear();
}

// One round with refine and verify on: graph scans of 6, 0, 3, 9 and 5 points; the new scan is
// scan 3's 9 points at (1, 2, 0.25); candidates 1 (empty: skipped), 2, 3, 4; rolling 10.
void check_loop_closure()
{
  ndt_2d_hip::LoopClosureHip lc(&the_matcher);
  const std::size_t sizes[5] = {6, 0, 3, 9, 5};
  for (std::size_t i = 0; i < 5; ++i)
  {
    std::size_t id = 99;
    CHECK(lc.storeScan(kPoints.data(), sizes[i], &id) && id == i);
  }
  settings.clear();
  CHECK(lc.setRefine(7, 0.5, 0.25, 9, 4));
  CHECK(lc.setVerify(4, 9, 9.0, 1.0, true));
  CHECK((settings == VecU{9u, 109u, 9001u, 201u}));
  VecD graph(15);
  for (std::size_t i = 0; i < graph.size(); ++i) graph[i] = 0.5 * static_cast<double>(i);
  double pose[3] = {1.0, 2.0, 0.25};
  const VecD scan(kPoints.begin() + 18, kPoints.end());
  std::vector<ndt_2d_hip::LoopClosure> closures;
  // round 1: candidates 2, 3, 4 -- 3 and 4 pass, 3 is accepted; round 2: 4 -- fails
  candidate_scores = {{-0.1, -0.9, -0.8}, {-0.1}};
  CHECK(lc.closeLoops(pose, scan.data(), 9, {1, 2, 3, 4}, graph.data(), 10, -0.5, 0, closures));
  CHECK(calls.size() == 4);
  if (calls.size() != 4) return;
  const Call & match = calls[0], & refine = calls[1], & verify = calls[2], & again = calls[3];
  const VecZ offsets = {0, 2, 4, 6}, ids = {1, 2, 2, 3, 3, 4};
  const VecD cand_poses = {1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0};
  CHECK(match.name == "match_candidates" && match.jobs == (VecD{1.0, 2.0, 0.25}) && match.points == scan);
  CHECK(match.n_candidates == 3 && match.cand_offsets == offsets && match.ids == ids && match.cand_poses == cand_poses);
  CHECK(!match.has_best && !match.has_all_scores && match.all_scores_cap == 0);
  // the refinement: the passing candidates 1 and 2 of the round as job_candidate, each from the scan's
  // pose + its correction, all on the one scan
  CHECK(refine.name == "refine_candidates" && refine.n_candidates == 3 && refine.cand_offsets == offsets && refine.ids == ids);
  CHECK(refine.cand_poses == cand_poses);
  CHECK(refine.n_jobs == 2 && refine.jobs == (VecD{2.0, 1.5, 0.5, 2.5, 1.25, 0.625}));
  CHECK(refine.has_job_scan && refine.job_scan == (VecU{0, 0}));
  CHECK(refine.has_job_candidate && refine.job_candidate == (VecU{1, 2}));
  CHECK(refine.n_scans == 1 && refine.offsets == (VecZ{0, 9}) && refine.points == scan);
  CHECK(refine.max_evals == 7 && refine.tol_lin == 0.5 && refine.tol_ang == 0.25 && !refine.has_gradients);
  // the verification: job 0 at its refined pose (usable), job 1 at its lattice pose (stalled)
  CHECK(verify.name == "verify_candidates" && verify.n_candidates == 3 && verify.cand_offsets == offsets && verify.ids == ids);
  CHECK(verify.cand_poses == cand_poses);
  CHECK(verify.n_jobs == 2 && verify.jobs == (VecD{2.0625, 1.5625, 0.5625, 2.5, 1.25, 0.625}));
  CHECK(verify.has_job_scan && verify.job_scan == (VecU{0, 0}));
  CHECK(verify.has_job_candidate && verify.job_candidate == (VecU{1, 2}));
  CHECK(verify.n_scans == 1 && verify.offsets == (VecZ{0, 9}) && verify.points == scan);
  CHECK(verify.max_beams == 4 && verify.cap == 0);
  CHECK(!verify.has_table && !verify.has_classes && !verify.has_m2 && !verify.has_cells);
  // the next round starts from the refined pose, on what is left
  CHECK(again.name == "match_candidates" && again.jobs == (VecD{2.0625, 1.5625, 0.5625}) && again.n_candidates == 1);
  CHECK(again.cand_offsets == (VecZ{0, 2}) && again.ids == (VecZ{3, 4}));
  CHECK(pose[0] == 2.0625 && pose[1] == 1.5625 && pose[2] == 0.5625);
  CHECK(closures.size() == 1);
  if (closures.size() != 1) return;
  const ndt_2d_hip::LoopClosure & c = closures[0];
  const double correction[3] = {1.0, -0.5, 0.25}, lattice[3] = {2.0, 1.5, 0.5}, refined[3] = {2.0625, 1.5625, 0.5625};
  const double cov4[9] = {1.0 / 7.0, -1.0 / 28.0, 0.0, -1.0 / 28.0, 1.0 / 14.0, 0.0, 0.0, 0.0, 1.0 / 32.0};
  CHECK(c.candidate == 3 && c.score == -0.9);
  for (int d = 0; d < 3; ++d)
  {
    CHECK(c.correction[d] == correction[d] && c.pose[d] == lattice[d]);
    CHECK(c.refined_pose[d] == refined[d] && c.verified_pose[d] == refined[d]);
  }
  for (int d = 0; d < 9; ++d) CHECK(c.covariance[d] == 9.0 + d && near(c.refined_covariance[d], cov4[d]));
  CHECK(c.refined && c.has_refined_covariance && c.refine_status == NDT2D_REFINE_CONVERGED && c.verified);
  const std::uint32_t record[8] = {4, 0, 1, 2, 3, 4, 5, 0};   // min(4, 9 points) beams
  for (int d = 0; d < 8; ++d) CHECK(c.verify[d] == record[d]);
  // a refusal in the round: false, the text
  calls.clear();
  candidate_scores = {{-0.9}};
  fail_next = true;
  CHECK(!lc.closeLoops(pose, scan.data(), 9, {4}, graph.data(), 10, -0.5, 0, closures) && closures.size() == 1);
  CHECK(lc.last_error() == "ndt2d error 3: canned refusal");
  fail_next = true;
  CHECK(!lc.setVerify(4, 9, 9.0, 1.0, true) && lc.last_error() == "ndt2d error 1: canned refusal");
  CHECK(lc.dropScans() && stored == 0);
  calls.clear();
}

}  // namespace

int main()
{
  check_track();
  check_refine();
  check_verify();
  check_relocalize();
  check_loop_closure();
  if (failures == 0) std::printf("OK\n");
  return failures == 0 ? 0 : 1;
}
