// The loop-closure thread's global optimisation (reference src/ndt_mapper.cpp:680,
// solver_->optimize(graph_->constraints, graph_->scans); src/ceres_solver.cpp:50-120) on
// libndt2d_hip.so: ndt2d_posegraph (include/ndt2d_hip.h, "Pose graph") -- Levenberg-Marquardt on
// the device, one launch, scans[0] held as the reference holds it.
//
// optimize(constraints, scans) has the shape of CeresSolver::optimize: it returns false for no
// scans or a failed solve and otherwise writes the corrected poses back into the scans.  It is a
// template over the node's own types and touches only what the reference's have:
//     constraint->begin, ->end, ->transform(i), ->information(i, j)           (ndt_2d::Constraint)
//     scan->getPose() with .x .y .theta, scan->setPose(pose)                   (ndt_2d::Scan, Pose2d)
// so nothing of ROS, Eigen or Ceres is included here; the overload on plain arrays is what it
// calls.  Unlike CeresSolver the whole problem is handed over at every call (no residual blocks
// are kept between calls), and a constraint whose information is not positive definite makes the
// call fail with a message that names it, where Eigen's llt() goes on silently.
//
// consistency(): the second use -- every switchable closure solved with and without: K masks over
// the one graph in one launch, chi2 of each closure against the solution of the others.  A verdict,
// no policy.
#ifndef NDT_2D_HIP__POSE_GRAPH_HIP_HPP_
#define NDT_2D_HIP__POSE_GRAPH_HIP_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// How one job ended.
struct PoseGraphRecord
{
  int status = NDT2D_POSEGRAPH_FAILED;   // NDT2D_POSEGRAPH_*
  std::uint32_t iterations = 0, cg_iterations = 0;
  double initial_cost = 0.0, final_cost = 0.0, gradient = 0.0;
  // of the "direct" and "sparse" solvers (cg_iterations is then 0): steps not taken, factorisations that failed
  // among them, the smallest pivot ratio of the last successful factorisation
  std::uint32_t rejected = 0, not_positive_definite = 0;
  double pivot_ratio = 0.0;
  bool usable() const { return status != NDT2D_POSEGRAPH_FAILED; }
};

class PoseGraphHip
{
public:
  explicit PoseGraphHip(ndt2d_matcher * matcher) : m_(matcher) {}
  PoseGraphHip(const PoseGraphHip &) = delete;
  PoseGraphHip & operator=(const PoseGraphHip &) = delete;
  ~PoseGraphHip()
  {
    dropCovariance();
    dropDirect();
    dropSparse();
    dropSparsecov();
    if (pg_ != nullptr) ndt2d_posegraph_destroy(pg_);
  }

  // Ceres's defaults (src/ceres_solver.cpp:39 and ceres::Solver::Options); a tolerance of 0
  // disables its rule.
  void setMaxIterations(std::uint32_t n) { max_iterations_ = n; }
  void setTolerances(double gradient, double function, double parameter)
  {
    gradient_tolerance_ = gradient;
    function_tolerance_ = function;
    parameter_tolerance_ = parameter;
  }
  // "reference": W = L as the reference passes it (the cost is e^T L^T L e); "information": W = L^T.
  void setWeighting(const std::string & weighting) { weighting_ = weighting; }
  // "jacobi" (the default) or "chain": the block-tridiagonal band of H + lambda D along the scans'
  // order, for the mapper's graphs (odometry between consecutive scans, a few closures).
  void setPreconditioner(const std::string & preconditioner) { preconditioner_ = preconditioner; }
  // What optimize() solves with: "cg" (the default: ndt2d_posegraph_solve, LM with a preconditioned CG
  // inside) or "direct" (ndt2d_direct_solve: the same LM rules with an exact step on a dense
  // Cholesky, whose cost does not depend on the closures; workspace_bytes: the device memory a
  // chunk's jobs may take, one 3n x 3n matrix of doubles a job) or "sparse" (ndt2d_sparse_solve: the
  // same exact step by a block cyclic reduction of the scans' chain and a Schur complement on the
  // scans closures touch, about 1 KiB a scan: for large maps with many closures).  false: another
  // name (last_error()).  consistency() keeps the CG solver.
  bool setSolver(const std::string & solver, std::size_t workspace_bytes = std::size_t(1) << 30)
  {
    if (solver != "cg" && solver != "direct" && solver != "sparse")
    {
      error_ = "setSolver: \"" + solver + "\" (\"cg\", \"direct\" or \"sparse\")";
      return false;
    }
    direct_solver_ = solver == "direct";
    sparse_solver_ = solver == "sparse";
    direct_workspace_ = workspace_bytes;
    return true;
  }
  // "trivial" (the default: the reference passes no loss function), "huber" or "cauchy" at `scale`,
  // applied to the switchable constraints (the closures): a gross outlier among them has almost no
  // pull on the poses.  The costs of the record are then the robust ones.
  void setLoss(const std::string & kind, double scale)
  {
    loss_ = kind;
    loss_scale_ = scale;
  }

  // Plain arrays: poses_xyt[n][3] in and out, constraints as ndt2d_posegraph_set_graph takes them.
  // false: no poses, a refused graph or a failed solve (last_error()); the poses stay then.
  // Called directly, a loss applies to every constraint (the arrays do not say which are switchable).
  bool optimize(double * poses_xyt, std::size_t n, const std::uint32_t * begin, const std::uint32_t * end, const double * transform,
                const double * information, std::size_t m)
  {
    record_ = PoseGraphRecord();
    if (n == 0) return false;   // `if (scans.empty()) return false;`
    if (!upload(poses_xyt, n, begin, end, transform, information, m, 1)) return false;
    return solve(poses_xyt, n);
  }

  // CeresSolver::optimize(constraints, scans): containers of (smart) pointers to the node's types.
  template <class Constraints, class Scans>
  bool optimize(const Constraints & constraints, Scans & scans)
  {
    record_ = PoseGraphRecord();
    if (!stage(constraints, scans, 1)) return false;   // `if (scans.empty()) return false;`
    if (!solve(poses_.data(), poses_.size() / 3)) return false;
    std::size_t i = 0;
    for (auto & scan : scans)
    {
      auto pose = scan->getPose();
      pose.x = poses_[3 * i];
      pose.y = poses_[3 * i + 1];
      pose.theta = poses_[3 * i + 2];
      scan->setPose(pose);
      ++i;
    }
    return true;
  }

  // Every switchable constraint solved without: job 0 has every constraint on, job 1 + k has the
  // k-th switchable constraint (in the order of `constraints`) off.  chi2_out[job][constraint] at
  // the job's solution; records_out per job.  The scans are not changed.
  template <class Constraints, class Scans>
  bool consistency(const Constraints & constraints, const Scans & scans, std::vector<std::vector<double>> & chi2_out,
                   std::vector<PoseGraphRecord> & records_out)
  {
    chi2_out.clear();
    records_out.clear();
    std::vector<std::size_t> switchable;
    std::size_t c = 0;
    for (const auto & constraint : constraints)
    {
      if (constraint->switchable) switchable.push_back(c);
      ++c;
    }
    const std::size_t jobs = 1 + switchable.size();
    if (!stage(constraints, scans, jobs)) return false;
    const std::size_t n = poses_.size() / 3, m = begin_.size();
    std::vector<std::uint8_t> enabled(jobs * m, 1);
    for (std::size_t k = 0; k < switchable.size(); ++k) enabled[(1 + k) * m + switchable[k]] = 0;
    out_.assign(jobs * 3 * n, 0.0);
    std::vector<double> rec(jobs * NDT2D_POSEGRAPH_RECORD_DOUBLES), chi2(jobs * 2 * m);
    if (!ok(ndt2d_posegraph_solve(pg_, enabled.data(), jobs, max_iterations_, gradient_tolerance_, function_tolerance_,
                                  parameter_tolerance_, out_.data(), rec.data(), chi2.data())))
    {
      return false;
    }
    for (std::size_t k = 0; k < jobs; ++k)
    {
      records_out.push_back(unpack(rec.data() + k * NDT2D_POSEGRAPH_RECORD_DOUBLES));
      chi2_out.emplace_back(chi2.begin() + (2 * k + 1) * m, chi2.begin() + (2 * k + 2) * m);
    }
    return true;
  }

  // Marginal covariances of chosen scans of the graph as it stands (include/ndt2d_hip.h, "Marginal
  // covariances"; scans[0] held, every constraint on, the loss set here on the switchable ones):
  // blocks_out[Q][Q][9], block (i, j) the rows of nodes[i] in the column of nodes[j]; status_out[Q]
  // NDT2D_MARGINALS_*.  false: no scans, a refused graph or call (last_error()).  The scans are not
  // changed; damping >= 0, 0 for the inverse itself.
  template <class Constraints, class Scans>
  bool marginals(const Constraints & constraints, const Scans & scans, const std::vector<std::uint32_t> & nodes,
                 std::vector<double> & blocks_out, std::vector<int> & status_out, double damping = 0.0, double tolerance = 1e-10)
  {
    blocks_out.clear();
    status_out.clear();
    const std::size_t q = nodes.size();
    if (!stage(constraints, scans, q > 0 ? q : 1)) return false;
    blocks_out.assign(q * q * 9, 0.0);
    std::vector<double> rec(q * NDT2D_MARGINALS_RECORD_DOUBLES, 0.0);
    if (!ok(ndt2d_marginals_columns(pg_, nullptr, 1, nullptr, nodes.data(), q, damping, tolerance, 0, blocks_out.data(), nullptr, rec.data())))
    {
      return false;
    }
    for (std::size_t i = 0; i < q; ++i) status_out.push_back(static_cast<int>(rec[i * NDT2D_MARGINALS_RECORD_DOUBLES]));
    return true;
  }

  // The predicted transform of scan b in scan a's frame with its covariance (transform_out[3],
  // covariance_out[9] row-major): marginals() of {a, b}, then ndt2d_marginals_relative.  false
  // also where a column did not converge (a component not joined to scans[0]).
  template <class Constraints, class Scans>
  bool relativeCovariance(const Constraints & constraints, const Scans & scans, std::uint32_t a, std::uint32_t b, double * transform_out,
                          double * covariance_out, double damping = 0.0, double tolerance = 1e-10)
  {
    std::vector<double> joint;
    std::vector<int> status;
    if (!marginals(constraints, scans, std::vector<std::uint32_t>{a, b}, joint, status, damping, tolerance)) return false;
    for (int s : status)
    {
      if (s != NDT2D_MARGINALS_CONVERGED && s != NDT2D_MARGINALS_NOT_FREE)
      {
        error_ = "ndt2d_marginals_columns: a column did not converge (status " + std::to_string(s) + ")";
        return false;
      }
    }
    return ok(ndt2d_marginals_relative(poses_.data() + 3 * a, poses_.data() + 3 * b, joint.data(), transform_out, covariance_out));
  }

  // The squared Mahalanobis distance of a proposed constraint (its transform, its information
  // inverted by the caller into covariance_meas[9]) from the graph's prediction for (begin, end)
  // as relativeCovariance gives it: against chi^2 with 3 degrees of freedom.  A verdict, no policy.
  template <class Constraints, class Scans>
  bool closureDistance(const Constraints & constraints, const Scans & scans, std::uint32_t begin, std::uint32_t end,
                       const double * transform_meas, const double * covariance_meas, double & d2_out)
  {
    double t[3], cov[9];
    if (!relativeCovariance(constraints, scans, begin, end, t, cov)) return false;
    return ok(ndt2d_marginals_distance(t, cov, transform_meas, covariance_meas, &d2_out));
  }

  // Every scan's 3 x 3 covariance and the blocks of chosen (a, b) pairs by a dense Cholesky on the
  // device (include/ndt2d_hip.h, "Dense covariance"; the graph as marginals() takes it), at a cost
  // that does not depend on the closures: diagonal_out[n][9], pairs_out[P][9] (the rows of scan a in
  // the columns of scan b) for pairs = {a0, b0, a1, b1, ...}.  false: no scans, a refused graph or
  // call, or a matrix that is not positive definite (a component not joined to scans[0] at
  // damping = 0); last_error() says which, pivotRatio() how close the factorisation came.
  // workspace_bytes: the device memory it may take, two 3 n x 3 n matrices of doubles.
  template <class Constraints, class Scans>
  bool covariances(const Constraints & constraints, const Scans & scans, const std::vector<std::uint32_t> & pairs,
                   std::vector<double> & diagonal_out, std::vector<double> & pairs_out, double damping = 0.0,
                   std::size_t workspace_bytes = std::size_t(1) << 30)
  {
    diagonal_out.clear();
    pairs_out.clear();
    if (!stage(constraints, scans, 1)) return false;
    const std::size_t n = poses_.size() / 3, p = pairs.size() / 2;
    const auto make = [&] {
      dropCovariance();
      return ndt2d_covariance_create(pg_, workspace_bytes, &cov_);
    };
    if (!companion(cov_, cov_bytes_, workspace_bytes, "ndt2d_covariance_create", make)) return false;
    diagonal_out.assign(n * 9, 0.0);
    pairs_out.assign(p * 9, 0.0);
    double rec[NDT2D_COVARIANCE_RECORD_DOUBLES] = {0.0, -1.0, 0.0};
    const int rc = ndt2d_covariance_compute(cov_, nullptr, 1, nullptr, damping, p != 0 ? pairs.data() : nullptr, p, diagonal_out.data(),
                                            p != 0 ? pairs_out.data() : nullptr, rec);
    if (rc != NDT2D_OK)
    {
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_covariance_last_error(cov_);
      return false;
    }
    pivot_ratio_ = rec[2];
    if (static_cast<int>(rec[0]) != NDT2D_COVARIANCE_OK)
    {
      error_ = "ndt2d_covariance_compute: not positive definite at unknown " + std::to_string(static_cast<long long>(rec[1]));
      return false;
    }
    return true;
  }

  // covariances() from the sparse solve's factorisation (include/ndt2d_hip.h, "Sparse covariance"): the
  // same arguments and outputs at O(n) + O(s^3) for s scans that closures touch, without a 3 n x 3 n
  // matrix -- for maps the dense call cannot hold.  false as covariances(); last_error() names the
  // stage (a pivot of the reduction, or of the Schur complement), pivotRatio() is the Schur
  // complement's (1 without a closure).
  template <class Constraints, class Scans>
  bool covariancesSparse(const Constraints & constraints, const Scans & scans, const std::vector<std::uint32_t> & pairs,
                         std::vector<double> & diagonal_out, std::vector<double> & pairs_out, double damping = 0.0,
                         std::size_t workspace_bytes = std::size_t(1) << 30)
  {
    diagonal_out.clear();
    pairs_out.clear();
    if (!stage(constraints, scans, 1)) return false;
    const std::size_t n = poses_.size() / 3, p = pairs.size() / 2;
    const auto make = [&] {
      dropSparsecov();
      return ndt2d_sparsecov_create(pg_, workspace_bytes, &sparsecov_);
    };
    if (!companion(sparsecov_, sparsecov_bytes_, workspace_bytes, "ndt2d_sparsecov_create", make)) return false;
    diagonal_out.assign(n * 9, 0.0);
    pairs_out.assign(p * 9, 0.0);
    double rec[NDT2D_COVARIANCE_RECORD_DOUBLES] = {0.0, 0.0, 0.0};
    const int rc = ndt2d_sparsecov_compute(sparsecov_, nullptr, 1, nullptr, damping, p != 0 ? pairs.data() : nullptr, p, diagonal_out.data(),
                                           p != 0 ? pairs_out.data() : nullptr, rec);
    if (rc != NDT2D_OK)
    {
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_sparsecov_last_error(sparsecov_);
      return false;
    }
    pivot_ratio_ = rec[2];
    if (static_cast<int>(rec[0]) != NDT2D_COVARIANCE_OK)
    {
      error_ = std::string("ndt2d_sparsecov_compute: not positive definite in a pivot of ") +
               (static_cast<int>(rec[1]) == 1 ? "the reduction" : "the Schur complement");
      return false;
    }
    return true;
  }

  double pivotRatio() const { return pivot_ratio_; }            // of the last covariances() or covariancesSparse()
  const PoseGraphRecord & record() const { return record_; }   // of the last optimize()
  const std::string & last_error() const { return error_; }

private:
  template <class Constraints>
  void gather(const Constraints & constraints)
  {
    begin_.clear();
    end_.clear();
    transform_.clear();
    information_.clear();
    robust_.clear();
    for (const auto & constraint : constraints)
    {
      robust_.push_back(constraint->switchable ? 1 : 0);
      begin_.push_back(static_cast<std::uint32_t>(constraint->begin));
      end_.push_back(static_cast<std::uint32_t>(constraint->end));
      for (int i = 0; i < 3; ++i) transform_.push_back(constraint->transform(i));
      for (int i = 0; i < 3; ++i)
      {
        for (int j = 0; j < 3; ++j) information_.push_back(constraint->information(i, j));
      }
    }
  }

  // What every call on the node's containers begins with: the scans' poses into poses_, the
  // constraints into the arrays, the graph on the device with room for `jobs`, and the loss's
  // selection (the switchable constraints).  false: no scans, or a refused graph (last_error()).
  template <class Constraints, class Scans>
  bool stage(const Constraints & constraints, const Scans & scans, std::size_t jobs)
  {
    poses_.clear();
    for (const auto & scan : scans)
    {
      const auto pose = scan->getPose();
      poses_.push_back(pose.x);
      poses_.push_back(pose.y);
      poses_.push_back(pose.theta);
    }
    gather(constraints);
    const std::size_t n = poses_.size() / 3, m = begin_.size();
    if (n == 0) return false;
    if (!upload(poses_.data(), n, begin_.data(), end_.data(), transform_.data(), information_.data(), m, jobs)) return false;
    if (m != 0 && !ok(ndt2d_robust_select(pg_, robust_.data(), m))) return false;
    robust_.clear();
    return true;
  }

  // One job, every constraint on, on the graph in place, by the solver chosen: record_, and the
  // poses into poses_xyt[n][3] where the solution is usable.
  bool solve(double * poses_xyt, std::size_t n)
  {
    out_.assign(3 * n, 0.0);
    if (direct_solver_)
    {
      if (!solveDirect()) return false;
    }
    else if (sparse_solver_)
    {
      if (!solveSparse()) return false;
    }
    else
    {
      double rec[NDT2D_POSEGRAPH_RECORD_DOUBLES];
      if (!ok(ndt2d_posegraph_solve(pg_, nullptr, 1, max_iterations_, gradient_tolerance_, function_tolerance_, parameter_tolerance_,
                                    out_.data(), rec, nullptr)))
      {
        return false;
      }
      record_ = unpack(rec);
    }
    if (!record_.usable()) return false;   // `if (!summary.IsSolutionUsable()) return false;`
    for (std::size_t i = 0; i < 3 * n; ++i) poses_xyt[i] = out_[i];
    return true;
  }

  // An object beside pg_ at a budget of workspace_bytes: made at its first use and again when the
  // budget changes, by make() -- the drop of the old one, then the ndt2d_<noun>_create named `create`.
  template <class T, class Make>
  bool companion(T * const & object, std::size_t & bytes, std::size_t workspace_bytes, const char * create, Make make)
  {
    if (object != nullptr && bytes == workspace_bytes) return true;
    const int rc = make();
    if (rc != NDT2D_OK)
    {
      error_ = "ndt2d error " + std::to_string(rc) + ": " + create;
      return false;
    }
    bytes = workspace_bytes;
    return true;
  }

  // The object (made anew when a capacity is passed) holding the graph.
  bool upload(const double * poses_xyt, std::size_t n, const std::uint32_t * begin, const std::uint32_t * end, const double * transform,
              const double * information, std::size_t m, std::size_t jobs)
  {
    if (pg_ == nullptr || n > max_nodes_ || m > max_constraints_ || jobs > max_jobs_)
    {
      dropCovariance();   // (they refer to the object that goes)
      dropDirect();
      dropSparse();
      dropSparsecov();
      if (pg_ != nullptr) ndt2d_posegraph_destroy(pg_);
      pg_ = nullptr;
      max_nodes_ = n > 2 * max_nodes_ ? n : 2 * max_nodes_;
      max_constraints_ = m > 2 * max_constraints_ ? m : 2 * max_constraints_;
      max_jobs_ = jobs > max_jobs_ ? (jobs < 65535 ? jobs : 65535) : max_jobs_;
      const int rc = ndt2d_posegraph_create(ndt2d_matcher_device(m_), max_nodes_, max_constraints_, max_jobs_, &pg_);
      if (rc != NDT2D_OK)
      {
        error_ = "ndt2d error " + std::to_string(rc) + ": ndt2d_posegraph_create";
        max_nodes_ = max_constraints_ = 0;
        max_jobs_ = 1;
        return false;
      }
    }
    if (!ok(ndt2d_posegraph_set_weighting(pg_, weighting_.c_str()))) return false;
    if (!ok(ndt2d_pose_graph_set_preconditioner(pg_, preconditioner_.c_str()))) return false;
    if (!ok(ndt2d_robust_set_loss(pg_, loss_.c_str(), loss_scale_))) return false;
    return ok(ndt2d_posegraph_set_graph(pg_, poses_xyt, n, begin, end, transform, information, m, 0));
  }

  static PoseGraphRecord unpack(const double * rec)
  {
    PoseGraphRecord r;
    r.status = static_cast<int>(rec[0]);
    r.iterations = static_cast<std::uint32_t>(rec[1]);
    r.cg_iterations = static_cast<std::uint32_t>(rec[2]);
    r.initial_cost = rec[3];
    r.final_cost = rec[4];
    r.gradient = rec[5];
    return r;
  }

  // One job, every constraint on, by ndt2d_direct_solve into out_ and record_.
  bool solveDirect()
  {
    const auto make = [&] {
      dropDirect();
      return ndt2d_direct_create(pg_, direct_workspace_, &direct_);
    };
    if (!companion(direct_, direct_bytes_, direct_workspace_, "ndt2d_direct_create", make)) return false;
    double rec[NDT2D_DIRECT_RECORD_DOUBLES];
    const int rc = ndt2d_direct_solve(direct_, nullptr, 1, max_iterations_, gradient_tolerance_, function_tolerance_, parameter_tolerance_,
                                      out_.data(), rec, nullptr);
    if (rc != NDT2D_OK)
    {
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_direct_last_error(direct_);
      return false;
    }
    record_ = unpackDirect(rec);
    return true;
  }

  // One job, every constraint on, by ndt2d_sparse_solve into out_ and record_.
  bool solveSparse()
  {
    const auto make = [&] {
      dropSparse();
      return ndt2d_sparse_create(pg_, direct_workspace_, &sparse_);
    };
    if (!companion(sparse_, sparse_bytes_, direct_workspace_, "ndt2d_sparse_create", make)) return false;
    double rec[NDT2D_DIRECT_RECORD_DOUBLES];
    const int rc = ndt2d_sparse_solve(sparse_, nullptr, 1, max_iterations_, gradient_tolerance_, function_tolerance_, parameter_tolerance_,
                                      out_.data(), rec, nullptr);
    if (rc != NDT2D_OK)
    {
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_sparse_last_error(sparse_);
      return false;
    }
    record_ = unpackDirect(rec);
    return true;
  }

  // The record of the two exact solvers.
  static PoseGraphRecord unpackDirect(const double * rec)
  {
    PoseGraphRecord r;
    r.status = static_cast<int>(rec[0]);
    r.iterations = static_cast<std::uint32_t>(rec[1]);
    r.rejected = static_cast<std::uint32_t>(rec[2]);
    r.not_positive_definite = static_cast<std::uint32_t>(rec[3]);
    r.initial_cost = rec[4];
    r.final_cost = rec[5];
    r.gradient = rec[6];
    r.pivot_ratio = rec[7];
    return r;
  }

  void dropDirect()
  {
    if (direct_ != nullptr) ndt2d_direct_destroy(direct_);
    direct_ = nullptr;
  }

  void dropSparse()
  {
    if (sparse_ != nullptr) ndt2d_sparse_destroy(sparse_);
    sparse_ = nullptr;
  }

  void dropSparsecov()
  {
    if (sparsecov_ != nullptr) ndt2d_sparsecov_destroy(sparsecov_);
    sparsecov_ = nullptr;
  }

  void dropCovariance()
  {
    if (cov_ != nullptr) ndt2d_covariance_destroy(cov_);
    cov_ = nullptr;
  }

  bool ok(int rc)
  {
    if (rc == NDT2D_OK) return true;
    error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_posegraph_last_error(pg_);
    return false;
  }

  ndt2d_matcher * m_;
  ndt2d_posegraph * pg_ = nullptr;
  ndt2d_covariance * cov_ = nullptr;   // made at the first covariances(), destroyed before pg_
  std::size_t cov_bytes_ = 0;
  ndt2d_direct * direct_ = nullptr;    // made at the first optimize() under "direct", destroyed before pg_
  std::size_t direct_bytes_ = 0, direct_workspace_ = std::size_t(1) << 30;
  bool direct_solver_ = false;
  ndt2d_sparse * sparse_ = nullptr;    // made at the first optimize() under "sparse", destroyed before pg_
  std::size_t sparse_bytes_ = 0;
  bool sparse_solver_ = false;
  ndt2d_sparsecov * sparsecov_ = nullptr;   // made at the first covariancesSparse(), destroyed before pg_
  std::size_t sparsecov_bytes_ = 0;
  double pivot_ratio_ = 0.0;
  std::size_t max_nodes_ = 0, max_constraints_ = 0, max_jobs_ = 1;
  std::uint32_t max_iterations_ = 100;
  double gradient_tolerance_ = 1e-10, function_tolerance_ = 1e-6, parameter_tolerance_ = 1e-8;
  std::string weighting_ = "reference", preconditioner_ = "jacobi", loss_ = "trivial";
  double loss_scale_ = 1.0;
  std::vector<double> poses_, transform_, information_, out_;
  std::vector<std::uint32_t> begin_, end_;
  std::vector<std::uint8_t> robust_;   // gather's: which constraints are switchable, until stage() has selected them
  PoseGraphRecord record_;
  std::string error_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__POSE_GRAPH_HIP_HPP_
