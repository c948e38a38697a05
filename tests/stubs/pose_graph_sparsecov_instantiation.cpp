// Compile-only use of ndt_2d_hip::PoseGraphHip::covariancesSparse beside covariances (ndt_2d_amd/plugin/pose_graph_hip.hpp)
// against include/ndt2d_hip.h, with stand-ins of its own for the reference's types as
// tests/stubs/pose_graph_instantiation.cpp has them.  Never linked or run.
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

int pose_graph_sparsecov_instantiation(ndt2d_matcher * matcher)
{
  std::vector<std::shared_ptr<stand_in::Scan>> scans;
  std::vector<std::shared_ptr<stand_in::Constraint>> constraints;
  for (int i = 0; i < 4; ++i)
  {
    scans.push_back(std::make_shared<stand_in::Scan>());
    auto c = std::make_shared<stand_in::Constraint>();
    c->begin = i;
    c->end = (i + 1) % 4;
    c->transform(0) = i < 3 ? 1.0 : -3.0;
    for (int j = 0; j < 3; ++j) c->information(j, j) = 100.0;
    c->switchable = i == 3;
    constraints.push_back(c);
  }
  ndt_2d_hip::PoseGraphHip solver(matcher);
  const std::vector<std::uint32_t> pairs = {1, 2, 2, 1, 3, 3};
  std::vector<double> diagonal, blocks, dense_diagonal, dense_blocks;
  if (!solver.covariancesSparse(constraints, scans, pairs, diagonal, blocks)) return 1;
  if (diagonal.size() != 36 || blocks.size() != 27 || !(solver.pivotRatio() > 0.0)) return 2;
  if (!solver.covariancesSparse(constraints, scans, pairs, diagonal, blocks, 1e-4, std::size_t(1) << 20)) return 3;
  // the same arguments and outputs as the dense call
  if (!solver.covariances(constraints, scans, pairs, dense_diagonal, dense_blocks, 1e-4, std::size_t(1) << 20)) return 4;
  return dense_diagonal.size() == diagonal.size() && dense_blocks.size() == blocks.size() ? 0 : 5;
}
