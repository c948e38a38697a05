// Stand-alone check of ndt_2d_amd/csrc/verify/ndt2d_verify_ray.h: the line walk and the closest
// approach the verification kernel's lanes run, on cases read from a file, printed for
// tests/test_verify_host.py to compare with the restatement.  Built with the host compiler (once
// more with -fsanitize=address,undefined) and run directly; no device, no library.
//
// The file:  G size_x size_y            then size_x * size_y records  "mx my i00 i01 i11 n"
//            R x y qx qy ox oy gx gy gate    a ray: the robot (x, y), the beam's end (qx, qy), the
//                                            origin cell, the end cell, gate_pierce
// doubles in C99 hexadecimal.  Per ray one line:
//            visited <flat cells> | tested <flat cells> | pierced <flat cell or -1> | rIr <hex per tested cell>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ndt2d_verify_ray.h"

namespace
{

struct Cell
{
  double mx, my, i00, i01, i11, n;
};

}  // namespace

int main(int argc, char ** argv)
{
  if (argc != 2)
  {
    std::fprintf(stderr, "usage: verify_ray_check CASES\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "r");
  if (f == nullptr)
  {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int size_x = 0, size_y = 0;
  if (std::fscanf(f, " G %d %d", &size_x, &size_y) != 2 || size_x <= 0 || size_y <= 0)
  {
    std::fprintf(stderr, "no grid\n");
    return 2;
  }
  std::vector<Cell> cells(static_cast<std::size_t>(size_x) * size_y);
  for (Cell & c : cells)
  {
    if (std::fscanf(f, "%la %la %la %la %la %la", &c.mx, &c.my, &c.i00, &c.i01, &c.i11, &c.n) != 6)
    {
      std::fprintf(stderr, "short grid\n");
      return 2;
    }
  }
  namespace V = ndt2d::verify;
  int rays = 0;
  for (;;)
  {
    double x, y, qx, qy, gate;
    int ox, oy, gx, gy;
    const int got = std::fscanf(f, " R %la %la %la %la %d %d %d %d %la", &x, &y, &qx, &qy, &ox, &oy, &gx, &gy, &gate);
    if (got == EOF) break;
    if (got != 9 || ox < 0 || oy < 0 || gx < 0 || gy < 0 || ox >= size_x || gx >= size_x || oy >= size_y || gy >= size_y)
    {
      std::fprintf(stderr, "bad ray %d\n", rays);
      return 2;
    }
    const double ux = qx - x, uy = qy - y;
    std::vector<long> visited, tested;
    std::vector<double> values;
    long pierced = -1;
    V::Line l = V::line_begin(ox, oy, gx, gy);
    const std::uint32_t max_cells = l.max_cells;
    for (std::uint32_t trip = 0; trip < max_cells; ++trip)
    {
      if (l.x < 0 || l.y < 0 || l.x >= size_x || l.y >= size_y)
      {
        std::printf("FAILED: ray %d leaves the grid\n", rays);
        return 1;
      }
      const long cell = static_cast<long>(l.y) * size_x + l.x;
      visited.push_back(cell);
      if (pierced < 0 && V::line_cell_testable(l, ox, oy) && cells[cell].n >= 5.0)
      {
        const Cell & c = cells[cell];
        const double rIr = V::approach(ux, uy, c.mx - x, c.my - y, c.i00, c.i01, c.i11);
        tested.push_back(cell);
        values.push_back(rIr);
        if (V::pierces(rIr, gate)) pierced = cell;
      }
      if (!V::line_next(l)) break;
    }
    std::printf("visited");
    for (long c : visited) std::printf(" %ld", c);
    std::printf(" | tested");
    for (long c : tested) std::printf(" %ld", c);
    std::printf(" | pierced %ld | rIr", pierced);
    for (double v : values) std::printf(" %a", v);
    std::printf("\n");
    ++rays;
  }
  std::fclose(f);
  std::printf("%d rays OK\n", rays);
  return 0;
}
