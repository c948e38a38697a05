// The synthetic workload generator (include/ndt2d_hip.h ndt2d_synth_*): a square room with a lattice
// of pillars, ray-cast scans with seeded noise.  Needs nothing else of the library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"

namespace
{

void guard_note(std::nullptr_t, const char *) noexcept {}   // (ndt2d_guard.h: these calls have no handle)

struct SplitMix64
{
  uint64_t s;
  explicit SplitMix64(uint64_t seed) : s(seed) {}
  uint64_t next()
  {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uniform() { return static_cast<double>(next() >> 11) * (1.0 / 9007199254740992.0); }
  double normal()
  {
    // Box-Muller, one value per two uniforms
    const double u1 = 1.0 - uniform();
    const double u2 = uniform();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
  }
};

bool pillar_in_cell(const ndt2d_world & w, long ci, long cj, double * cx, double * cy)
{
  *cx = w.pillar_pitch * static_cast<double>(ci) + 0.5 * w.pillar_pitch;
  *cy = w.pillar_pitch * static_cast<double>(cj) + 0.5 * w.pillar_pitch;
  return std::fabs(*cx) + w.pillar_half < w.room_half && std::fabs(*cy) + w.pillar_half < w.room_half;
}

// Distance along (dx, dy) from (ox, oy) to the nearest surface.
double raycast(const ndt2d_world & w, double ox, double oy, double dx, double dy)
{
  const double inf = std::numeric_limits<double>::infinity();
  // room walls (origin inside the room)
  double t_wall = inf;
  if (dx > 0) t_wall = std::min(t_wall, (w.room_half - ox) / dx);
  if (dx < 0) t_wall = std::min(t_wall, (-w.room_half - ox) / dx);
  if (dy > 0) t_wall = std::min(t_wall, (w.room_half - oy) / dy);
  if (dy < 0) t_wall = std::min(t_wall, (-w.room_half - oy) / dy);
  if (!(w.pillar_pitch > 0.0) || !(w.pillar_half > 0.0)) return t_wall;

  // walk the pillar lattice cells the ray crosses (one pillar per cell)
  const double pitch = w.pillar_pitch;
  long ci = static_cast<long>(std::floor(ox / pitch));
  long cj = static_cast<long>(std::floor(oy / pitch));
  const long step_i = dx > 0 ? 1 : -1, step_j = dy > 0 ? 1 : -1;
  double t_max_x = dx != 0 ? ((dx > 0 ? (ci + 1) * pitch : ci * pitch) - ox) / dx : inf;
  double t_max_y = dy != 0 ? ((dy > 0 ? (cj + 1) * pitch : cj * pitch) - oy) / dy : inf;
  const double t_dx = dx != 0 ? pitch / std::fabs(dx) : inf;
  const double t_dy = dy != 0 ? pitch / std::fabs(dy) : inf;
  double t_enter = 0.0;
  while (t_enter <= t_wall)
  {
    double cx, cy;
    if (pillar_in_cell(w, ci, cj, &cx, &cy))
    {
      // slab test against [cx - h, cx + h] x [cy - h, cy + h]
      double t0 = 0.0, t1 = inf;
      bool hit = true;
      const double lo[2] = {cx - w.pillar_half, cy - w.pillar_half};
      const double hi[2] = {cx + w.pillar_half, cy + w.pillar_half};
      const double o[2] = {ox, oy}, d[2] = {dx, dy};
      for (int a = 0; a < 2 && hit; ++a)
      {
        if (d[a] == 0.0)
        {
          if (o[a] < lo[a] || o[a] > hi[a]) hit = false;
        }
        else
        {
          double ta = (lo[a] - o[a]) / d[a], tb = (hi[a] - o[a]) / d[a];
          if (ta > tb) std::swap(ta, tb);
          t0 = std::max(t0, ta);
          t1 = std::min(t1, tb);
          if (t0 > t1) hit = false;
        }
      }
      if (hit && t0 > 0.0 && t0 < t_wall) return t0;
    }
    if (t_max_x < t_max_y)
    {
      t_enter = t_max_x;
      t_max_x += t_dx;
      ci += step_i;
    }
    else
    {
      t_enter = t_max_y;
      t_max_y += t_dy;
      cj += step_j;
    }
  }
  return t_wall;
}

}  // namespace

extern "C" {

int ndt2d_synth_scan(const ndt2d_world * world, const double * pose_xyt, size_t n_beams,
                     double noise_sigma, uint64_t seed, double * points_xy)
{
  NDT2D_C_TRY
  if (world == nullptr || pose_xyt == nullptr || points_xy == nullptr || n_beams == 0)
  {
    return NDT2D_ERR_INVALID;
  }
  if (std::fabs(pose_xyt[0]) >= world->room_half || std::fabs(pose_xyt[1]) >= world->room_half)
  {
    return NDT2D_ERR_INVALID;
  }
  SplitMix64 rng(seed);
  const double step = 2.0 * M_PI / static_cast<double>(n_beams);
  for (size_t k = 0; k < n_beams; ++k)
  {
    const double ang = -M_PI + static_cast<double>(k) * step;
    const double wa = pose_xyt[2] + ang;
    double r = raycast(*world, pose_xyt[0], pose_xyt[1], std::cos(wa), std::sin(wa));
    r += noise_sigma * rng.normal();
    points_xy[2 * k] = r * std::cos(ang);
    points_xy[2 * k + 1] = r * std::sin(ang);
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_synth_pose_blocked(const ndt2d_world * world, double x, double y, double margin)
{
  NDT2D_C_TRY
  if (world == nullptr || !(world->pillar_pitch > 0.0)) return 0;
  const long ci = static_cast<long>(std::floor(x / world->pillar_pitch));
  const long cj = static_cast<long>(std::floor(y / world->pillar_pitch));
  double cx, cy;
  if (!pillar_in_cell(*world, ci, cj, &cx, &cy)) return 0;
  return (std::fabs(x - cx) <= world->pillar_half + margin &&
          std::fabs(y - cy) <= world->pillar_half + margin)
           ? 1
           : 0;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_synth_uniform(uint64_t seed, size_t n, double * out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  SplitMix64 rng(seed);
  for (size_t i = 0; i < n; ++i) out[i] = rng.uniform();
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

}  // extern "C"
