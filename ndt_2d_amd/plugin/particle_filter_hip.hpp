// ndt_2d::ParticleFilter with the particle set resident in GPU memory.
//
// Same constructor arguments and methods as the reference's filter
// (include/ndt_2d/particle_filter.hpp:49-115, src/particle_filter.cpp), over the
// C-ABI of libndt2d_hip.so (include/ndt2d_hip.h): init / update / measure and
// every updateStatistics run as HIP kernels on one device array that lives as
// long as the filter; resample keeps the reference's sequential KLD stopping rule
// on the host (src/particle_filter.cpp:91-140).
//
// Differences a maintainer should know:
//  * The reference draws its noise from an mt19937 seeded by std::random_device
//    (motion_model.hpp:63-64); here the draws come from the device's counter-based
//    stream, keyed by an explicit `seed` and one step per init / update call, so
//    runs are reproducible.  resample() keeps an mt19937 (std::discrete_distribution
//    over the weights, :94), seeded from the same `seed`.
//  * The KD-tree of the reference (kd_tree.hpp) is only asked for its leaf count
//    (:118); the library's ndt2d_kld_resample counts the distinct discrete keys
//    (kd_tree.hpp:95-98), which is the same number.
//  * No Eigen in this header: getMean / getCovariance fill plain arrays (row-major
//    3 x 3), so that it builds without ROS; scan_matcher_ndt_hip.cpp style adaptors
//    to Eigen::Vector3d / Matrix3d are two lines.
//
// Error behaviour follows the reference: no exceptions; ok() turns false on the
// first failed device call and last_error() tells why.
#ifndef NDT_2D_HIP__PARTICLE_FILTER_HIP_HPP_
#define NDT_2D_HIP__PARTICLE_FILTER_HIP_HPP_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "clearance_hip.hpp"
#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// One pose cluster as bestCluster() reports it: getMean()- and getCovariance()-shaped values from
// the cluster's particles only (row-major 3 x 3; only [8] is filled for theta, as the filter fills
// it), and its share W / W_total of the set's weight.
struct PoseClusterHip
{
  double mean[3] = {0.0, 0.0, 0.0};
  double covariance[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double share = 0.0;
  std::uint32_t label = 0, count = 0;
};

class ParticleFilterHip
{
public:
  // MotionModel(a1..a5) (include/ndt_2d/motion_model.hpp:52) folded in as alphas5.
  ParticleFilterHip(std::size_t min_particles, std::size_t max_particles, const double * alphas5,
                    ndt2d_matcher * matcher, std::uint64_t seed = 0)
  : matcher_(matcher),
    dev_(ndt2d_matcher_device(matcher)),
    min_particles_(min_particles),
    max_particles_(max_particles),
    seed_(seed),
    gen_(static_cast<std::mt19937::result_type>(seed))
  {
    std::copy(alphas5, alphas5 + 5, alphas_);
    // particles_.assign(min_particles_, (0, 0, 0)); weights_ = 1 / min (src/particle_filter.cpp:48-50)
    resize(min_particles_);
    std::vector<double> zeros(3 * n_, 0.0), w(n_, n_ ? 1.0 / static_cast<double>(n_) : 0.0);
    check(ndt2d_copy_to_device(dev_, d_particles_, zeros.data(), zeros.size() * sizeof(double)));
    check(ndt2d_copy_to_device(dev_, d_weights_, w.data(), w.size() * sizeof(double)));
    updateStatistics(false);
  }

  ~ParticleFilterHip()
  {
    if (seeder_ != nullptr) ndt2d_seed_destroy(seeder_);
    clearance_.reset();
    if (clusterer_ != nullptr) ndt2d_cluster_destroy(clusterer_);
    ndt2d_device_free(dev_, d_count_);
    ndt2d_device_free(dev_, d_particles_);
    ndt2d_device_free(dev_, d_weights_);
    ndt2d_device_free(dev_, d_stats_);
  }

  ParticleFilterHip(const ParticleFilterHip &) = delete;
  ParticleFilterHip & operator=(const ParticleFilterHip &) = delete;

  // src/particle_filter.cpp:53-69
  void init(double x, double y, double theta, double sigma_x, double sigma_y, double sigma_theta)
  {
    check(ndt2d_pf_init_launch(dev_, d_particles_, n_, x, y, theta, sigma_x, sigma_y, sigma_theta,
                               nullptr, seed_, ++step_, 0));
    std::vector<double> w(n_, 1.0 / static_cast<double>(n_));
    check(ndt2d_copy_to_device(dev_, d_weights_, w.data(), w.size() * sizeof(double)));
    updateStatistics(false);
  }

  // src/particle_filter.cpp:71-76
  void update(double dx, double dy, double dth)
  {
    check(ndt2d_pf_motion_launch(dev_, d_particles_, n_, dx, dy, dth, alphas_, nullptr, seed_,
                                 ++step_, 0));
    updateStatistics(false);
  }

  // src/particle_filter.cpp:78-89; points = scan->getPoints(), interleaved x, y
  void measure(const double * points_xy, std::size_t n_points)
  {
    std::size_t n_beams = 0;
    check(ndt2d_matcher_prepare_beams(matcher_, points_xy, n_points, &n_beams));
    if (!ok_) return;
    if (!ndt2d_matcher_has_ndt(matcher_) || n_beams == 0)
    {
      // scorePoints returns 0.0 without a map (src/scan_matcher_ndt.cpp:159), 0.0 / 0 without points
      std::vector<double> w(n_, n_beams == 0 && ndt2d_matcher_has_ndt(matcher_) ? std::nan("") : 0.0);
      check(ndt2d_copy_to_device(dev_, d_weights_, w.data(), w.size() * sizeof(double)));
      updateStatistics(false);
      return;
    }
    check(ndt2d_score_poses_launch(dev_, d_particles_, n_, d_weights_, d_stats_));
    updateStatistics(true);
  }

  // src/particle_filter.cpp:91-140
  void resample(double kld_err, double kld_z)
  {
    std::vector<double> particles(3 * n_), weights(n_);
    check(ndt2d_copy_to_host(dev_, particles.data(), d_particles_, particles.size() * sizeof(double)));
    check(ndt2d_copy_to_host(dev_, weights.data(), d_weights_, weights.size() * sizeof(double)));
    if (!ok_) return;
    // the draws of std::discrete_distribution (:94,110) as uniforms from the same
    // mt19937; the draw-and-stop loop (:107-133) is the library's host code
    std::vector<double> uniforms(max_particles_);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    for (double & u : uniforms) u = unit(gen_);
    // KD-tree leaf size 0.5 x 0.5 x 0.2671 (particle_filter.cpp:44)
    const double leaf[3] = {0.5, 0.5, 0.2671};
    std::vector<std::uint32_t> chosen(std::max<std::size_t>(max_particles_, 1));
    std::size_t n_kept = 0;
    check(ndt2d_kld_resample(particles.data(), weights.data(), n_, min_particles_, max_particles_,
                             kld_err, kld_z, leaf, uniforms.data(), uniforms.size(), chosen.data(),
                             &n_kept));
    if (!ok_) return;
    std::vector<double> resampled, resampled_weights;
    resampled.reserve(3 * n_kept);
    resampled_weights.reserve(n_kept);
    for (std::size_t i = 0; i < n_kept; ++i)
    {
      const std::size_t p = chosen[i];
      resampled.insert(resampled.end(), particles.begin() + 3 * p, particles.begin() + 3 * p + 3);
      resampled_weights.push_back(weights[p]);
    }
    resize(resampled_weights.size());
    check(ndt2d_copy_to_device(dev_, d_particles_, resampled.data(), resampled.size() * sizeof(double)));
    check(ndt2d_copy_to_device(dev_, d_weights_, resampled_weights.data(),
                               resampled_weights.size() * sizeof(double)));
    updateStatistics(false);
  }

  // Global localisation (not in the reference; include/ndt2d_hip.h "Global localisation"): the set
  // becomes n particles (0 = max_particles) uniform over the free cells (byte 0) of a HOST
  // row-major int8 map, heading uniform, weights 1 / n.  region4 = {x0, y0, w, h} in cells or
  // nullptr.  Consumes two steps of the counter; the map stays this filter's free table for inject.
  // min_clearance > 0 (metres, the robot's radius) keeps only the free cells at least that far from
  // every obstacle of the whole map ("Clearance map": bytes that are neither 0 nor -1); 0.0 is the
  // call without it.
  void initGlobal(const signed char * map, std::uint32_t width, std::uint32_t height, double origin_x,
                  double origin_y, double resolution, std::size_t n = 0,
                  const std::uint32_t * region4 = nullptr, double min_clearance = 0.0)
  {
    if (!seeder()) return;
    if (min_clearance != 0.0)
    {
      const signed char * d_masked = cleared(map, false, width, height, resolution, min_clearance);
      if (!ok_) return;
      seedCheck(ndt2d_seed_set_map_device(seeder_, d_masked, width, height, origin_x, origin_y, resolution, region4));
    }
    else
    {
      seedCheck(ndt2d_seed_set_map(seeder_, map, width, height, origin_x, origin_y, resolution, region4));
    }
    seedFrom(n);
  }
  // The same from the resident map of an ndt2d_occupancy_map's last update: nothing is uploaded.
  void initGlobal(ndt2d_occupancy_map * resident, std::size_t n = 0, const std::uint32_t * region4 = nullptr,
                  double min_clearance = 0.0)
  {
    if (!seeder()) return;
    const signed char * d_map = nullptr;
    ndt2d_occupancy_info info;
    check(ndt2d_occmap_device_map(resident, &d_map, &info));
    if (!ok_) return;
    if (min_clearance != 0.0) d_map = cleared(d_map, true, info.width, info.height, info.resolution, min_clearance);
    if (!ok_) return;
    seedCheck(ndt2d_seed_set_map_device(seeder_, d_map, info.width, info.height, info.origin_x, info.origin_y,
                                        info.resolution, region4));
    seedFrom(n);
  }

  // Augmented MCL's recovery step: every particle is replaced, with `probability`, by a fresh sample
  // over the free table of the last initGlobal.  Weights are not touched.  Consumes two steps;
  // returns the number replaced.
  std::size_t inject(double probability)
  {
    if (seeder_ == nullptr && ok_)
    {
      ok_ = false;
      error_ = "inject: no free table, call initGlobal first";
    }
    if (!ok_) return 0;
    if (d_count_ == nullptr)
    {
      void * p = nullptr;
      check(ndt2d_device_alloc(dev_, sizeof(std::uint64_t), &p));
      d_count_ = static_cast<std::uint64_t *>(p);
    }
    if (!ok_) return 0;
    const std::uint64_t step = step_ + 1;
    step_ += 2;
    seedCheck(ndt2d_seed_inject_launch(seeder_, d_particles_, n_, probability, seed_, step, 0, d_count_));
    std::uint64_t replaced = 0;
    check(ndt2d_copy_to_host(dev_, &replaced, d_count_, sizeof(replaced)));
    updateStatistics(false);
    return ok_ ? static_cast<std::size_t>(replaced) : 0;
  }

  // Pose clusters (not in the reference; include/ndt2d_hip.h "Pose clusters"): the set as it stands
  // grouped on the device into connected clusters of occupied pose bins; the max_clusters (1 .. 16)
  // heaviest, heaviest first.  getMean / getCovariance are not touched.  The records are this
  // object's until the next call; clusterHeader() is that call's header.
  const std::vector<ndt2d_cluster_record> & clusters(int max_clusters = 8)
  {
    records_.clear();
    cluster_header_ = ndt2d_cluster_header();
    if (!clusterer()) return records_;
    clusterCheck(ndt2d_cluster_set_max_clusters(clusterer_, max_clusters));
    if (ok_) clusterCheck(ndt2d_cluster_launch(clusterer_, d_particles_, d_weights_, n_));
    if (!ok_) return records_;
    records_.resize(NDT2D_CLUSTER_MAX_RECORDS);
    std::size_t found = 0;
    clusterCheck(ndt2d_cluster_fetch(clusterer_, &cluster_header_, records_.data(), records_.size(), &found));
    records_.resize(ok_ ? found : 0);
    return records_;
  }
  const ndt2d_cluster_header & clusterHeader() const { return cluster_header_; }

  // The heaviest cluster: where a node that started with initGlobal reads its pose instead of
  // getMean() while the set still has several modes.  false when no particle belongs to a cluster.
  bool bestCluster(PoseClusterHip * out)
  {
    const std::vector<ndt2d_cluster_record> & found = clusters(1);
    if (!ok_ || found.empty() || out == nullptr) return false;
    const ndt2d_cluster_record & r = found.front();
    *out = PoseClusterHip();
    out->mean[0] = r.mean_x;
    out->mean[1] = r.mean_y;
    out->mean[2] = r.mean_theta;
    out->covariance[0] = r.cxx;
    out->covariance[1] = out->covariance[3] = r.cxy;
    out->covariance[4] = r.cyy;
    out->covariance[8] = r.var_theta;
    out->share = cluster_header_.w_total > 0.0 ? r.weight / cluster_header_.w_total : 0.0;
    out->label = r.label;
    out->count = r.count;
    return true;
  }

  void getMean(double * mean3) const { std::copy(mean_, mean_ + 3, mean3); }
  void getCovariance(double * cov9) const { std::copy(cov_, cov_ + 9, cov9); }

  std::size_t size() const { return n_; }
  // Host copy of the particles ({x, y, theta} triples), e.g. for getMsg (:152-161).
  std::vector<double> particles()
  {
    std::vector<double> out(3 * n_);
    check(ndt2d_copy_to_host(dev_, out.data(), d_particles_, out.size() * sizeof(double)));
    return out;
  }
  std::vector<double> weights()
  {
    std::vector<double> out(n_);
    check(ndt2d_copy_to_host(dev_, out.data(), d_weights_, out.size() * sizeof(double)));
    return out;
  }
  std::uint64_t step() const { return step_; }

  bool ok() const { return ok_; }
  const std::string & last_error() const { return error_; }

private:
  void check(int rc)
  {
    if (rc != NDT2D_OK && ok_)
    {
      ok_ = false;
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_last_error(dev_);
    }
  }

  bool seeder()
  {
    if (seeder_ == nullptr && ok_) check(ndt2d_seed_create(dev_, &seeder_));
    return ok_;
  }

  // This filter's masked DEVICE copy of a map: the free cells nearer than min_clearance to an obstacle
  // are 99 in it.  The transform is capped at the radius the clearance needs, so it costs at most that
  // many steps a cell however open the map is.
  const signed char * cleared(const signed char * map, bool on_device, std::uint32_t width, std::uint32_t height,
                              double resolution, double min_clearance)
  {
    std::uint32_t min_d2 = 0;
    if (!ClearanceMapHip::minD2(min_clearance, resolution, 0, &min_d2))
    {
      ok_ = false;
      error_ = "initGlobal: min_clearance and the resolution do not give a clearance in cells";
      return nullptr;
    }
    const std::int64_t cap = static_cast<std::int64_t>(std::ceil(min_clearance / resolution));   // cap^2 >= min_d2
    if (!clearance_) clearance_.reset(new ClearanceMapHip(dev_));
    const signed char * d_masked = nullptr;
    if (clearance_->valid() && (on_device ? clearance_->computeDevice(map, width, height, false, cap)
                                          : clearance_->compute(map, width, height, false, cap)))
    {
      d_masked = clearance_->mask(min_d2);
    }
    if (d_masked == nullptr && ok_)
    {
      ok_ = false;
      error_ = clearance_->last_error();
    }
    return d_masked;
  }

  // created on first use, for the largest set this filter can hold
  bool clusterer()
  {
    if (clusterer_ != nullptr && cluster_capacity_ < n_ && ok_)
    {
      ndt2d_cluster_destroy(clusterer_);
      clusterer_ = nullptr;
    }
    if (clusterer_ == nullptr && ok_)
    {
      cluster_capacity_ = std::max<std::size_t>(std::max(capacity_, n_), 1);
      check(ndt2d_cluster_create(dev_, cluster_capacity_, &clusterer_));
    }
    return ok_;
  }

  void clusterCheck(int rc)
  {
    if (rc != NDT2D_OK && ok_)
    {
      ok_ = false;
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_cluster_last_error(clusterer_);
    }
  }

  void seedCheck(int rc)
  {
    if (rc != NDT2D_OK && ok_)
    {
      ok_ = false;
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_seed_last_error(seeder_);
    }
  }

  // n fresh particles from the seeder's table, weights 1 / n, statistics
  void seedFrom(std::size_t n)
  {
    if (!ok_) return;
    if (n == 0) n = max_particles_;
    resize(n);
    if (!ok_ || n_ == 0) return;
    const std::uint64_t step = step_ + 1;
    step_ += 2;
    seedCheck(ndt2d_seed_launch(seeder_, d_particles_, n_, seed_, step, 0));
    std::vector<double> w(n_, 1.0 / static_cast<double>(n_));
    check(ndt2d_copy_to_device(dev_, d_weights_, w.data(), w.size() * sizeof(double)));
    updateStatistics(false);
  }

  void resize(std::size_t n)
  {
    if (n > capacity_)
    {
      ndt2d_device_free(dev_, d_particles_);
      ndt2d_device_free(dev_, d_weights_);
      d_particles_ = d_weights_ = nullptr;
      capacity_ = std::max(n, max_particles_);
      void * p = nullptr;
      check(ndt2d_device_alloc(dev_, 3 * capacity_ * sizeof(double), &p));
      d_particles_ = static_cast<double *>(p);
      check(ndt2d_device_alloc(dev_, capacity_ * sizeof(double), &p));
      d_weights_ = static_cast<double *>(p);
    }
    if (d_stats_ == nullptr)
    {
      void * p = nullptr;
      check(ndt2d_device_alloc(dev_, (NDT2D_POSE_STATS_DOUBLES + NDT2D_PF_RESULT_DOUBLES) * sizeof(double), &p));
      d_stats_ = static_cast<double *>(p);
    }
    n_ = n;
  }

  // src/particle_filter.cpp:163-218 on the device; have_moments: the sums were just
  // written by ndt2d_score_poses_launch
  void updateStatistics(bool have_moments)
  {
    if (n_ == 0 || !ok_) return;
    if (!have_moments) check(ndt2d_pose_moments_launch(dev_, d_particles_, n_, d_weights_, d_stats_));
    double * d_out = d_stats_ + NDT2D_POSE_STATS_DOUBLES;
    check(ndt2d_pf_finalize_launch(dev_, d_particles_, n_, d_weights_, d_stats_, d_out));
    double out[NDT2D_PF_RESULT_DOUBLES];
    check(ndt2d_copy_to_host(dev_, out, d_out, sizeof(out)));
    if (!ok_) return;
    mean_[0] = out[1];
    mean_[1] = out[2];
    mean_[2] = out[3];
    cov_[0] = out[4];
    cov_[1] = cov_[3] = out[5];
    cov_[4] = out[6];
    cov_[8] += out[7];   // never zeroed by the reference either (:216)
  }

  ndt2d_matcher * matcher_;
  ndt2d_handle dev_;
  std::size_t min_particles_, max_particles_;
  double alphas_[5];
  std::uint64_t seed_, step_ = 0;
  std::mt19937 gen_;
  double * d_particles_ = nullptr, * d_weights_ = nullptr, * d_stats_ = nullptr;
  ndt2d_seeder * seeder_ = nullptr;
  std::unique_ptr<ClearanceMapHip> clearance_;   // made by the first initGlobal with a clearance
  ndt2d_clusterer * clusterer_ = nullptr;
  std::size_t cluster_capacity_ = 0;
  ndt2d_cluster_header cluster_header_ = ndt2d_cluster_header();
  std::vector<ndt2d_cluster_record> records_;
  std::uint64_t * d_count_ = nullptr;
  std::size_t n_ = 0, capacity_ = 0;
  double mean_[3] = {0.0, 0.0, 0.0};
  double cov_[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok_ = true;
  std::string error_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__PARTICLE_FILTER_HIP_HPP_
