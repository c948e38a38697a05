// Host-only check of the layout of one chunk's upload in the batched searches on the installed
// grid (ndt_2d_amd/csrc/batch/ndt2d_stage_layout.h): [dth | dlin | beams | jobs | order | cos /
// sin rows].  For every case the beams start on a 16-byte boundary, the pieces follow each other
// without overlap, the order table's odd half lies inside the stage and the total is the sum of
// the parts; then a buffer of exactly that size is filled piece by piece as match_chunk fills
// it, so that a miscounted offset is a report of the address sanitizer this is built with.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ndt2d_stage_layout.h"

static int bad = 0;

static void expect(bool ok, const char * what)
{
  if (!ok)
  {
    std::printf("FAILED: %s\n", what);
    ++bad;
  }
}

// record: kJobDoubles with an order table (jobs) or kStartDoubles without one (start poses)
static void check_case(size_t n_th, size_t n_lin, size_t n_beams, size_t n_slots, size_t n_rows, size_t record)
{
  const bool ordered = record == ndt2d::kJobDoubles;
  const size_t trig = n_rows * 2 * n_th;
  const ndt2d::StageLayout l = ndt2d::stage_layout(n_th, n_lin, n_beams, n_slots, record, ordered ? n_slots : 0, trig);
  const size_t order_doubles = ordered ? (n_slots + 1) / 2 : 0;   // two 32-bit entries to a double
  const size_t pad = (n_th + n_lin) % 2;            // in front of the beams

  expect(l.dth == 0 && l.dlin == l.dth + n_th, "dth, then dlin");
  expect(l.beams == l.dlin + n_lin + pad, "the beams follow dlin, one double of padding at most");
  expect((l.beams * sizeof(double)) % 16 == 0, "the beams start on a 16-byte boundary");
  expect(l.jobs == l.beams + 2 * n_beams, "the jobs follow the beams");
  expect(l.order == l.jobs + n_slots * record, "the order table follows the jobs");
  expect(l.trig == l.order + order_doubles, "the rows follow the order table");
  expect(l.total == l.trig + trig, "the rows end the stage");
  expect(l.total == n_th + n_lin + pad + 2 * n_beams + n_slots * record + order_doubles + trig,
         "the total is the sum of the parts");
  expect(l.dth < l.dlin && l.dlin < l.beams && l.beams < l.jobs && l.jobs < l.order && l.order <= l.trig && l.trig < l.total &&
             (l.order < l.trig) == ordered,
         "the pieces are in order and none but an absent order table is empty");
  // the double the host zeroes for an odd last entry: inside the order table, hence inside the stage
  if (ordered) expect(l.trig - 1 >= l.order && l.trig - 1 < l.total, "the order table's odd half lies inside the stage");
  if (ordered) expect(n_slots * sizeof(uint32_t) <= order_doubles * sizeof(double), "the order entries fit their doubles");

  // exactly l.total doubles, filled as match_chunk fills them
  std::vector<double> stage(l.total, -1.0);
  double * st = stage.data();
  const std::vector<double> dth(n_th, 1.0), dlin(n_lin, 2.0), beams(2 * n_beams, 3.0), jobs(n_slots * record, 4.0),
      rows(trig, 6.0);
  const std::vector<uint32_t> order(ordered ? n_slots : 0, 0x40140000u);   // (the high word of 5.0)
  std::memcpy(st + l.dth, dth.data(), n_th * sizeof(double));
  std::memcpy(st + l.dlin, dlin.data(), n_lin * sizeof(double));
  std::memcpy(st + l.beams, beams.data(), 2 * n_beams * sizeof(double));
  std::memcpy(st + l.jobs, jobs.data(), n_slots * record * sizeof(double));
  if (ordered) st[l.trig - 1] = 0.0;
  if (ordered) std::memcpy(st + l.order, order.data(), n_slots * sizeof(uint32_t));
  std::memcpy(st + l.trig, rows.data(), trig * sizeof(double));
  // every double was written by its own piece and by no other; only the padding keeps the fill
  size_t untouched = 0;
  for (size_t i = 0; i < l.total; ++i)
  {
    const double want = i < l.dlin ? 1.0 : i < l.dlin + n_lin ? 2.0 : i < l.beams ? -1.0 : i < l.jobs ? 3.0 : i < l.order ? 4.0 : 6.0;
    if (i >= l.order && i < l.trig) continue;   // (32-bit entries: below)
    if (stage[i] != want) expect(false, "a piece overwrote its neighbour");
    if (stage[i] == -1.0) ++untouched;
  }
  expect(untouched == pad, "only the padding is left unwritten");
  std::vector<uint32_t> back(2 * order_doubles);
  if (ordered) std::memcpy(back.data(), st + l.order, order_doubles * sizeof(double));
  for (size_t j = 0; j < back.size(); ++j) expect(back[j] == (j < order.size() ? 0x40140000u : 0u), "order entries, the odd half zeroed");
}

int main()
{
  size_t n_cases = 0;
  const size_t lattices[][2] = {{1, 7}, {3, 7}, {80, 21}, {80, 20}, {1, 1}, {2, 1}};   // n_th + n_lin even and odd
  for (const auto & lat : lattices)
  {
    for (size_t n_slots : {1, 2, 5})
    {
      for (size_t n_beams : {1, 1500})
      {
        for (size_t n_rows : {1, 3})
        {
          check_case(lat[0], lat[1], n_beams, n_slots, n_rows, ndt2d::kJobDoubles);
          check_case(lat[0], lat[1], n_beams, n_slots, n_rows, ndt2d::kStartDoubles);
          n_cases += 2;
        }
      }
    }
  }
  std::printf("%zu cases\n", n_cases);
  std::printf(bad == 0 ? "OK\n" : "FAILED\n");
  return bad == 0 ? 0 : 1;
}
