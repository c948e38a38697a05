// Compile-only use of ndt_2d_hip::PoseGraphHip (ndt_2d_amd/plugin/pose_graph_hip.hpp) against
// include/ndt2d_hip.h, with stand-ins of its own for what the reference's types offer it
// (ndt_2d::Constraint: begin, end, transform(i), information(i, j), switchable; ndt_2d::Scan:
// getPose() / setPose(); Pose2d: x, y, theta).  Never linked or run.
#include <memory>
#include <vector>

#include "../../ndt_2d_amd/plugin/pose_graph_hip.hpp"

namespace stand_in
{

// (the members of Eigen::Vector3d / Matrix3d the mirror uses)
struct Vector3
{
  double v[3] = {0.0, 0.0, 0.0};
  double & operator()(int i) { return v[i]; }
  double operator()(int i) const { return v[i]; }
};

struct Matrix3
{
  double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double & operator()(int i, int j) { return v[3 * i + j]; }
  double operator()(int i, int j) const { return v[3 * i + j]; }
};

struct Pose2d
{
  double x = 0.0, y = 0.0, theta = 0.0;
};

struct Constraint
{
  int begin = 0, end = 0;
  Vector3 transform;
  Matrix3 information;
  bool switchable = false;
};

class Scan
{
public:
  Pose2d getPose() const { return pose_; }
  void setPose(const Pose2d & pose) { pose_ = pose; }

private:
  Pose2d pose_;
};

}  // namespace stand_in

int pose_graph_instantiation(ndt2d_matcher * matcher)
{
  using ConstraintPtr = std::shared_ptr<stand_in::Constraint>;
  using ScanPtr = std::shared_ptr<stand_in::Scan>;
  std::vector<ScanPtr> scans;
  std::vector<ConstraintPtr> constraints;
  ndt_2d_hip::PoseGraphHip solver(matcher);
  if (solver.optimize(constraints, scans)) return 1;   // no scans: false, as the reference
  for (int i = 0; i < 3; ++i)
  {
    scans.push_back(std::make_shared<stand_in::Scan>());
    stand_in::Pose2d pose;
    pose.x = i;
    scans.back()->setPose(pose);
  }
  for (int i = 0; i < 3; ++i)
  {
    ConstraintPtr c = std::make_shared<stand_in::Constraint>();
    c->begin = i;
    c->end = (i + 1) % 3;
    c->transform(0) = i < 2 ? 1.0 : -1.9;
    for (int j = 0; j < 3; ++j) c->information(j, j) = 100.0;
    c->switchable = i == 2;
    constraints.push_back(c);
  }
  solver.setMaxIterations(50);
  solver.setTolerances(1e-10, 1e-6, 1e-8);
  solver.setWeighting("information");
  if (!solver.optimize(constraints, scans)) return 2;
  if (!solver.record().usable() || solver.record().final_cost > solver.record().initial_cost) return 3;
  std::vector<std::vector<double>> chi2;
  std::vector<ndt_2d_hip::PoseGraphRecord> records;
  if (!solver.consistency(constraints, scans, chi2, records)) return 4;
  if (records.size() != 2 || chi2.size() != 2 || chi2[1].size() != 3) return 5;
  // the plain arrays, and the C entry points themselves
  double poses[6] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  const std::uint32_t begin[1] = {0}, end[1] = {1};
  const double transform[3] = {1.1, 0.0, 0.0}, information[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  if (!solver.optimize(poses, 2, begin, end, transform, information, 1)) return 6;
  ndt2d_posegraph * pg = nullptr;
  if (ndt2d_posegraph_create(ndt2d_matcher_device(matcher), 2, 1, 1, &pg) != NDT2D_OK) return 7;
  double cost = 0.0, chi2_one[1], residuals[6], out[6], record[NDT2D_POSEGRAPH_RECORD_DOUBLES], chi2_two[2];
  float kernel_ms = 0.0f, fetch_ms = 0.0f;
  const std::uint8_t enabled[1] = {1};
  const bool fine = ndt2d_posegraph_set_weighting(pg, "reference") == NDT2D_OK && ndt2d_posegraph_weighting(pg)[0] == 'r' &&
                    ndt2d_posegraph_set_graph(pg, poses, 2, begin, end, transform, information, 1, 0) == NDT2D_OK &&
                    ndt2d_posegraph_set_timing(pg, 1) == NDT2D_OK &&
                    ndt2d_posegraph_evaluate(pg, enabled, 1, &cost, chi2_one, residuals) == NDT2D_OK &&
                    ndt2d_posegraph_solve(pg, enabled, 1, 100, 1e-10, 1e-6, 1e-8, out, record, chi2_two) == NDT2D_OK &&
                    ndt2d_posegraph_last_ms(pg, &kernel_ms, &fetch_ms) == NDT2D_OK && ndt2d_posegraph_last_error(pg) != nullptr;
  return ndt2d_posegraph_destroy(pg) == NDT2D_OK && fine && record[0] != NDT2D_POSEGRAPH_FAILED ? 0 : 8;
}
