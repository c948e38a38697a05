// Host-only check of the dense covariance's plan (ndt_2d_amd/csrc/covariance/ndt2d_covariance_plan.h),
// exhaustive for d = 3 ... 300 and for 3,069 / 3,072 / 3,075: the padding, the launch list walked as
// the device runs it -- every lower block behind a panel updated exactly once per panel, every block
// of T left of and below a panel exactly once, the substitutions' workgroups covering their rows and
// columns, no index beyond the padded matrix -- the index of an unknown, the triangle's numbering
// and the chunk size from a byte budget.  Prints what it counted; the last line is "ok".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ndt2d_covariance_plan.h"

namespace cov = ndt2d::covariance;

static int bad = 0;

static void expect(bool ok, const char * what, size_t d)
{
  if (ok) return;
  ++bad;
  if (bad <= 20) std::printf("FAILED at d = %zu: %s\n", d, what);
}

static void check_dimension(size_t d)
{
  const size_t np = cov::panels(d), ld = cov::padded(d);
  expect(ld >= d && ld < d + cov::kPanel && ld % cov::kPanel == 0 && ld == np * cov::kPanel, "padding", d);
  expect(cov::kPanel % 3 == 0 && cov::kPanel % cov::kTile == 0, "a node's block or a tile straddles a panel", d);
  std::vector<cov::Launch> list(cov::launch_list(d, nullptr));
  expect(cov::launch_list(d, list.data()) == list.size(), "the count and the list", d);
  // how often each block was updated behind the current panel
  std::vector<int> hits(np * np);
  size_t at = 0;
  for (int phase = 0; phase < 2; ++phase)
  {
    for (uint32_t p = 0; p < np; ++p)
    {
      const size_t below = np - p - 1;
      // the factor or the row solve
      expect(at < list.size() && list[at].panel == p && list[at].groups != 0, "a panel's first launch", d);
      if (phase == 0)
      {
        expect(list[at].kind == cov::kFactor && list[at].groups == 1, "one workgroup factors the diagonal block", d);
        ++at;
        if (below != 0)
        {
          expect(at < list.size() && list[at].kind == cov::kSolveBelow && list[at].panel == p, "the panel below", d);
          const size_t rows = below * cov::kPanel, covered = static_cast<size_t>(list[at].groups) * cov::kRows;
          expect(covered >= rows && covered < rows + cov::kRows, "the rows below are covered once", d);
          expect((p + 1) * cov::kPanel + rows == ld, "the last row is the matrix's last", d);
          ++at;
        }
      }
      else
      {
        expect(list[at].kind == cov::kSolveRow, "the row of T", d);
        const size_t cols = (p + 1) * static_cast<size_t>(cov::kPanel), covered = static_cast<size_t>(list[at].groups) * cov::kRows;
        expect(covered >= cols && covered < cols + cov::kRows && cols <= ld, "the columns of the row are covered once", d);
        ++at;
      }
      if (below == 0) continue;
      const int kind = phase == 0 ? cov::kUpdate : cov::kUpdateRect;
      expect(at < list.size() && list[at].kind == kind && list[at].panel == p, "the update", d);
      std::fill(hits.begin(), hits.end(), 0);
      for (uint32_t g = 0; g < list[at].groups; ++g)
      {
        uint32_t bi = 0, bj = 0;
        cov::update_block(kind, p, g, &bi, &bj);
        expect(bi < np && bj < np, "a block beyond the matrix", d);
        if (bi < np && bj < np) ++hits[bi * np + bj];
      }
      for (uint32_t bi = 0; bi < np; ++bi)
      {
        for (uint32_t bj = 0; bj < np; ++bj)
        {
          const bool wanted = phase == 0 ? (bi > p && bj > p && bj <= bi) : (bi > p && bj <= p);
          expect(hits[bi * np + bj] == (wanted ? 1 : 0), "a block updated not exactly once, or one that must stay", d);
        }
      }
      ++at;
    }
  }
  expect(at == list.size(), "launches left over", d);
  if (d % 3 == 0)
  {
    const size_t n = d / 3;
    expect(cov::unknown(n - 1, 2) == d - 1 && cov::unknown(0, 0) == 0 && cov::unknown(n - 1, 0) / cov::kPanel == cov::unknown(n - 1, 2) / cov::kPanel,
           "a node's unknowns", d);
    expect(cov::job_doubles(n) == 2 * ld * ld + ld + 3 * n, "a job's doubles", d);
    // the chunk from a budget
    const size_t bytes = cov::job_doubles(n) * sizeof(double);
    expect(cov::chunk_jobs(8, bytes - 1, bytes) == 0 && cov::chunk_jobs(8, bytes, bytes) == 1 && cov::chunk_jobs(8, 3 * bytes + 7, bytes) == 3 &&
             cov::chunk_jobs(8, 100 * bytes, bytes) == 8 && cov::chunk_jobs(1, 100 * bytes, bytes) == 1,
           "the chunk size", d);
  }
}

int main()
{
  size_t checked = 0;
  for (size_t d = 3; d <= 300; ++d, ++checked) check_dimension(d);
  for (size_t d : {size_t(3069), size_t(3072), size_t(3075)})
  {
    check_dimension(d);
    ++checked;
  }
  // the triangle's numbering, every q of 2,000 rows and the largest rows a matrix can have
  uint64_t q = 0;
  for (uint32_t r = 0; r < 2000; ++r)
  {
    for (uint32_t c = 0; c <= r; ++c, ++q)
    {
      uint32_t gr = 0, gc = 0;
      cov::lower_tile(q, &gr, &gc);
      if (gr != r || gc != c) expect(false, "lower_tile", q);
    }
  }
  const uint32_t rows = static_cast<uint32_t>(cov::panels(cov::kMaxDim));
  for (uint32_t r = rows - 3; r < rows; ++r)
  {
    for (uint32_t c : {0u, 1u, r - 1, r})
    {
      uint32_t gr = 0, gc = 0;
      cov::lower_tile(cov::lower_tiles(r) + c, &gr, &gc);
      if (gr != r || gc != c) expect(false, "lower_tile at the largest dimension", r);
    }
  }
  expect(cov::lower_tiles(rows) < (uint64_t(1) << 31) && cov::kMaxDim % cov::kPanel == 0 && cov::kMaxDim <= 65535, "the grid's limits", cov::kMaxDim);
  std::printf("dimensions %zu, panels of 3075: %zu, launches of 3075: %zu, padded(3069 / 3072 / 3075): %zu %zu %zu\n", checked, cov::panels(3075),
              cov::launch_list(3075, nullptr), cov::padded(3069), cov::padded(3072), cov::padded(3075));
  std::printf(bad == 0 ? "ok\n" : "FAILED\n");
  return bad == 0 ? 0 : 1;
}
