// Compile-only use of ndt_2d_hip::PoseGraphHip::setLoss (ndt_2d_amd/plugin/pose_graph_hip.hpp)
// against include/ndt2d_hip.h: a loss on the container overload (the switchable constraints), on
// the plain-array overload (every constraint) and in consistency(), with stand-ins of its own for
// the reference's types as tests/stubs/pose_graph_instantiation.cpp has them.  Never linked or run.
#include <cstdint>
#include <memory>
#include <vector>

#include "../../ndt_2d_amd/plugin/pose_graph_hip.hpp"

namespace stand_in
{

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

int pose_graph_loss_instantiation(ndt2d_matcher * matcher)
{
  std::vector<std::shared_ptr<stand_in::Scan>> scans;
  std::vector<std::shared_ptr<stand_in::Constraint>> constraints;
  for (int i = 0; i < 3; ++i)
  {
    scans.push_back(std::make_shared<stand_in::Scan>());
    auto c = std::make_shared<stand_in::Constraint>();
    c->begin = i;
    c->end = (i + 1) % 3;
    c->transform(0) = i < 2 ? 1.0 : -5.0;   // (the closure disagrees grossly)
    for (int j = 0; j < 3; ++j) c->information(j, j) = 100.0;
    c->switchable = i == 2;
    constraints.push_back(c);
  }
  ndt_2d_hip::PoseGraphHip solver(matcher);
  solver.setLoss("huber", 1.5);
  if (!solver.optimize(constraints, scans)) return 1;
  solver.setLoss("cauchy", 2.0);
  std::vector<std::vector<double>> chi2;
  std::vector<ndt_2d_hip::PoseGraphRecord> records;
  if (!solver.consistency(constraints, scans, chi2, records)) return 2;
  double poses[6] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  const std::uint32_t begin[1] = {0}, end[1] = {1};
  const double transform[3] = {1.1, 0.0, 0.0}, information[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  solver.setLoss("trivial", 1.0);
  if (!solver.optimize(poses, 2, begin, end, transform, information, 1)) return 3;
  double rho3[3];
  return ndt2d_robust_rho("huber", 1.5, solver.record().final_cost, rho3) == NDT2D_OK ? 0 : 4;
}
