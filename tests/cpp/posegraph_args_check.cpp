// Host-only check of what the pose-graph calls refuse about their arguments
// (ndt_2d_amd/csrc/posegraph/ndt2d_posegraph_args.h): every refusal's text, written out here as the
// entry points gave it before the header held it, and the empty string for every acceptable input.
// The dense limits come from ndt_2d_amd/csrc/covariance/ndt2d_covariance_plan.h as the entry points
// pass them.  A program of its own, built with the host compiler, plainly and with the sanitizers.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "ndt2d_covariance_plan.h"
#include "ndt2d_posegraph_args.h"

using namespace ndt2d::pg_args;
namespace cov = ndt2d::covariance;

static int bad = 0;

static void expect(const std::string & got, const char * want, const char * what)
{
  if (got != want)
  {
    std::printf("FAILED: %s: \"%s\", not \"%s\"\n", what, got.c_str(), want);
    ++bad;
  }
}

static std::string dense(const char * entry, size_t n, size_t max_jobs, size_t workspace_bytes)
{
  const size_t job_bytes = cov::job_doubles(n) * sizeof(double);
  return dense_refusal(entry, n, cov::kMaxDim, cov::chunk_jobs(max_jobs, workspace_bytes, job_bytes), job_bytes, workspace_bytes);
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  // ---- the poses of n_jobs jobs of n nodes: the first offender, its job i / (3 n), its pose i / 3 % n ----
  {
    const size_t jobs = 3, n = 5;
    std::vector<double> poses(jobs * n * 3, 0.25);
    expect(poses_refusal("ndt2d_marginals_columns", nullptr, jobs, n), "", "no poses");
    expect(poses_refusal("ndt2d_marginals_columns", poses.data(), jobs, n), "", "finite poses");
    expect(poses_refusal("ndt2d_marginals_columns", poses.data(), 0, n), "", "no jobs");
    poses[(0 * n + 2) * 3 + 1] = inf;
    expect(poses_refusal("ndt2d_marginals_columns", poses.data(), jobs, n), "ndt2d_marginals_columns: job 0 pose 2 is not finite", "job 0 pose 2");
    expect(poses_refusal("ndt2d_covariance_compute", poses.data(), jobs, n), "ndt2d_covariance_compute: job 0 pose 2 is not finite",
           "job 0 pose 2, the covariance's");
    poses[(0 * n + 2) * 3 + 1] = 0.25;
    poses[(2 * n + 4) * 3 + 2] = nan;    // the last value of all
    expect(poses_refusal("ndt2d_covariance_compute", poses.data(), jobs, n), "ndt2d_covariance_compute: job 2 pose 4 is not finite", "job 2 pose 4");
    poses[(1 * n + 0) * 3 + 0] = -inf;   // in front of it: the first offender is named
    expect(poses_refusal("ndt2d_covariance_compute", poses.data(), jobs, n), "ndt2d_covariance_compute: job 1 pose 0 is not finite", "job 1 pose 0");
    expect(poses_refusal("ndt2d_covariance_compute", poses.data(), 1, n), "", "the first job alone");
  }

  // ---- the damping ----
  expect(damping_refusal("ndt2d_marginals_columns", 0.0), "", "damping 0");
  expect(damping_refusal("ndt2d_marginals_columns", -0.0), "", "damping -0");
  expect(damping_refusal("ndt2d_marginals_columns", 1e300), "", "a large damping");
  expect(damping_refusal("ndt2d_marginals_columns", -1e-9), "ndt2d_marginals_columns: the damping is negative or not finite", "damping < 0");
  expect(damping_refusal("ndt2d_marginals_columns", nan), "ndt2d_marginals_columns: the damping is negative or not finite", "damping NaN");
  expect(damping_refusal("ndt2d_covariance_compute", inf), "ndt2d_covariance_compute: the damping is negative or not finite", "damping inf");
  expect(damping_refusal("ndt2d_covariance_compute", -inf), "ndt2d_covariance_compute: the damping is negative or not finite", "damping -inf");

  // ---- the three tolerances, each in turn ----
  expect(tolerances_refusal("ndt2d_posegraph_solve", 0.0, 0.0, 0.0), "", "tolerances 0");
  expect(tolerances_refusal("ndt2d_posegraph_solve", 1e-10, 1e-6, 1e-8), "", "the defaults");
  for (int which = 0; which < 3; ++which)
  {
    double t[3] = {1e-10, 1e-6, 1e-8};
    t[which] = -0.0;
    expect(tolerances_refusal("ndt2d_direct_solve", t[0], t[1], t[2]), "", "a tolerance of -0");
    for (const double v : {nan, inf, -inf, -1e-300})
    {
      t[which] = v;
      expect(tolerances_refusal("ndt2d_posegraph_solve", t[0], t[1], t[2]), "ndt2d_posegraph_solve: a tolerance is negative or not finite",
             "a bad tolerance, the solver's");
      expect(tolerances_refusal("ndt2d_direct_solve", t[0], t[1], t[2]), "ndt2d_direct_solve: a tolerance is negative or not finite",
             "a bad tolerance, the direct solve's");
    }
  }

  // ---- node ids against n ----
  {
    const uint32_t queries[4] = {0, 6, 7, 9};
    expect(nodes_refusal("ndt2d_marginals_columns", "query", queries, 2, 1, 7), "", "queries below n");
    expect(nodes_refusal("ndt2d_marginals_columns", "query", queries, 0, 1, 7), "", "no queries");
    expect(nodes_refusal("ndt2d_marginals_columns", "query", queries, 4, 1, 7), "ndt2d_marginals_columns: query 2 names node 7 of 7", "a query of n");
    expect(nodes_refusal("ndt2d_marginals_columns", "query", queries, 4, 1, 8), "ndt2d_marginals_columns: query 3 names node 9 of 8", "a query past n");
    const uint32_t pairs[6] = {1, 3, 4, 0, 2, 5};
    expect(nodes_refusal("ndt2d_covariance_compute", "pair", pairs, 3, 2, 6), "", "pairs below n");
    expect(nodes_refusal("ndt2d_covariance_compute", "pair", pairs, 3, 2, 4), "ndt2d_covariance_compute: pair 1 names node 4 of 4", "a pair's first of n");
    expect(nodes_refusal("ndt2d_covariance_compute", "pair", pairs, 3, 2, 5), "ndt2d_covariance_compute: pair 2 names node 5 of 5", "a pair's second of n");
    expect(nodes_refusal("ndt2d_covariance_compute", "pair", pairs, 1, 2, 4), "", "the first pair alone");
  }

  // ---- the dense limits ----
  {
    const size_t fits = cov::kMaxDim / 3;   // 3 n = kMaxDim
    expect(dense("ndt2d_covariance_compute", fits, 4, ~size_t(0)), "", "3 n = kMaxDim");
    expect(dense("ndt2d_covariance_compute", fits + 1, 4, ~size_t(0)), "ndt2d_covariance_compute: 21841 poses, a dense matrix holds 21840",
           "3 n = kMaxDim + 3");
    expect(dense("ndt2d_direct_solve", fits + 1, 4, 1), "ndt2d_direct_solve: 21841 poses, a dense matrix holds 21840", "the dimension before the budget");
    const size_t need = 8 * (2 * 48 * 48 + 48 + 12);   // a job of 4 poses: one panel
    expect(dense("ndt2d_covariance_compute", 4, 2, need), "", "a budget of one job");
    expect(dense("ndt2d_covariance_compute", 4, 2, need - 1), "ndt2d_covariance_compute: a job of 4 poses needs 37344 bytes, the workspace is 37343",
           "a budget one byte short of one job");
    expect(dense_refusal("ndt2d_direct_solve", 4, cov::kMaxDim, cov::chunk_jobs(2, 99, 100), 100, 99),
           "ndt2d_direct_solve: a job of 4 poses needs 100 bytes, the workspace is 99", "the direct solve's bytes");
    expect(dense_refusal("ndt2d_direct_solve", 4, cov::kMaxDim, cov::chunk_jobs(2, 100, 100), 100, 100), "", "the direct solve's bytes, held");
  }

  if (bad != 0) return 1;
  std::printf("ok\n");
  return 0;
}
