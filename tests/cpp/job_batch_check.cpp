// The (scan, pose) job list of the matcher's batched calls (ndt_2d_amd/csrc/host/ndt2d_job_batch.h),
// a program of its own over the plain-C++ header, linked with host/ndt2d_host_ndt.cpp for
// subsample_into: built with the host compiler and the sanitizers, run directly
// (tests/test_job_list_host.py).  The expected values are written out by hand.  Prints OK, or FAILED
// lines.
//
// The one list: 5 jobs over 4 scans of 6, 0, 3 and 9 points, limit 4; jobs 0 and 3 share scan 0,
// scan 1 is empty, scan 2 is shorter than the limit, scan 3 longer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "host/ndt2d_job_batch.h"

using namespace ndt2d::host;

static int failures = 0;

#define CHECK(cond)                                                      \
  do                                                                     \
  {                                                                      \
    if (!(cond))                                                         \
    {                                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

using VecD = std::vector<double>;
using VecZ = std::vector<size_t>;
using VecU = std::vector<uint32_t>;

// Scan s, point i: (10 s + i, 10 s + i + 0.5).
static const VecD kPoints = {0.0,  0.5,  1.0,  1.5,  2.0,  2.5,  3.0,  3.5,  4.0,  4.5,  5.0,  5.5,    // scan 0: 6
                                                                                                       // scan 1: 0
                             20.0, 20.5, 21.0, 21.5, 22.0, 22.5,                                        // scan 2: 3
                             30.0, 30.5, 31.0, 31.5, 32.0, 32.5, 33.0, 33.5, 34.0, 34.5, 35.0, 35.5, 36.0, 36.5, 37.0, 37.5,
                             38.0, 38.5};                                                               // scan 3: 9
static const VecZ kOffsets = {0, 6, 6, 9, 18};
static const VecD kJobs = {1.0, 2.0, 0.25, 3.0, 4.0, 0.5, 5.0, 6.0, 0.75, 7.0, 8.0, 1.0, 9.0, 10.0, 1.25};
static const VecU kJobScan = {0, 1, 2, 0, 3};
constexpr uint32_t kEmpty = ~0u - 1u;

// 4 of 6 points: indices 0, 1 (1.5), 3, 4 (4.5); 4 of 9: 0, 2 (2.25), 4 (4.5), 6 (6.75)
static const VecD kScan0Of4 = {0.0, 0.5, 1.0, 1.5, 3.0, 3.5, 4.0, 4.5};
static const VecD kScan2 = {20.0, 20.5, 21.0, 21.5, 22.0, 22.5};
static const VecD kScan3Of4 = {30.0, 30.5, 32.0, 32.5, 34.0, 34.5, 36.0, 36.5};
static const VecD kBatchJobs = {1.0, 2.0, 0.25, 5.0, 6.0, 0.75, 7.0, 8.0, 1.0, 9.0, 10.0, 1.25};   // jobs 0, 2, 3, 4

static VecD joined(std::initializer_list<VecD> parts)
{
  VecD out;
  for (const VecD & p : parts) out.insert(out.end(), p.begin(), p.end());
  return out;
}

// A scan's part of the batch is subsample_into of that scan alone.
static void check_alone(const JobBatch & b, size_t sent, const double * points, size_t n_points, size_t limit)
{
  VecD one;
  subsample_into(one, points, n_points, limit);
  CHECK(b.scan_beams(sent) == one.size() / 2);
  CHECK(VecD(b.beams.begin() + 2 * b.beam_offsets[sent], b.beams.begin() + 2 * b.beam_offsets[sent + 1]) == one);
}

static void check_collection()
{
  // job_scan given: scan 0 once for jobs 0 and 3; scan 1 and its job 1 stay out
  JobBatch b;
  collect_job_batch(4, kJobs.data(), kJobScan.data(), 5, kPoints.data(), kOffsets.data(), 4, b);
  CHECK(b.size() == 4 && b.scans() == 3);
  CHECK((b.job == VecU{0, 2, 3, 4}) && (b.scan == VecU{0, 1, 0, 2}));
  CHECK((b.sent == VecU{0, kEmpty, 1, 2}));
  CHECK((b.beam_offsets == VecZ{0, 4, 7, 11}));
  CHECK(b.beams == joined({kScan0Of4, kScan2, kScan3Of4}));
  CHECK(b.xyt == kBatchJobs);
  check_alone(b, 0, kPoints.data(), 6, 4);
  check_alone(b, 1, kPoints.data() + 12, 3, 4);
  check_alone(b, 2, kPoints.data() + 18, 9, 4);
  CHECK(b.beams_of(0) == 4 && b.beams_of(1) == 3 && b.beams_of(2) == 4 && b.beams_of(3) == 4);
  CHECK(batch_beams(b) == 15);
  // the verification's offsets table: job 1, of the empty scan, takes no room
  VecZ table(6, 99);
  fill_verify_offsets(b, 5, table.data());
  CHECK((table == VecZ{0, 4, 4, 7, 11, 15}));

  // no job_scan: the equivalent list of 5 scans (scan 0's points twice), job k on scan k
  const VecD points5 = joined({VecD(kPoints.begin(), kPoints.begin() + 12), kScan2, VecD(kPoints.begin(), kPoints.begin() + 12),
                               VecD(kPoints.begin() + 18, kPoints.end())});
  const VecZ offsets5 = {0, 6, 6, 9, 15, 24};
  JobBatch c;
  collect_job_batch(4, kJobs.data(), nullptr, 5, points5.data(), offsets5.data(), 5, c);
  CHECK(c.size() == 4 && c.scans() == 4);
  CHECK((c.job == VecU{0, 2, 3, 4}) && (c.scan == VecU{0, 1, 2, 3}));
  CHECK((c.sent == VecU{0, kEmpty, 1, 2, 3}));
  CHECK((c.beam_offsets == VecZ{0, 4, 7, 11, 15}));
  CHECK(c.beams == joined({kScan0Of4, kScan2, kScan0Of4, kScan3Of4}));
  CHECK(c.xyt == kBatchJobs);
  check_alone(c, 2, points5.data() + 18, 6, 4);
  CHECK(batch_beams(c) == 15);
  fill_verify_offsets(c, 5, table.data());
  CHECK((table == VecZ{0, 4, 4, 7, 11, 15}));

  // limit 0 as it is (match_scans): no scan has beams, no job is in the batch
  JobBatch none;
  collect_job_batch(0, kJobs.data(), kJobScan.data(), 5, kPoints.data(), kOffsets.data(), 4, none);
  CHECK(none.size() == 0 && none.scans() == 0 && none.beams.empty() && none.xyt.empty());
  CHECK((none.sent == VecU{kEmpty, kEmpty, kEmpty, kEmpty}) && (none.beam_offsets == VecZ{0}));
  CHECK(batch_beams(none) == 0);
  fill_verify_offsets(none, 5, table.data());
  CHECK((table == VecZ{0, 0, 0, 0, 0, 0}));
  // limit 0 as "every point" (the registrations, the verifications)
  JobBatch all;
  collect_job_batch(kEveryPoint, kJobs.data(), kJobScan.data(), 5, kPoints.data(), kOffsets.data(), 4, all);
  CHECK(all.size() == 4 && (all.beam_offsets == VecZ{0, 6, 9, 18}) && all.beams == kPoints);
  CHECK((all.job == VecU{0, 2, 3, 4}) && (all.scan == VecU{0, 1, 0, 2}));
  CHECK(batch_beams(all) == 24);
  fill_verify_offsets(all, 5, table.data());
  CHECK((table == VecZ{0, 6, 6, 9, 15, 24}));
  // a scan no job names is not subsampled
  const VecU two = {3, 3};
  JobBatch d;
  collect_job_batch(4, kJobs.data(), two.data(), 2, kPoints.data(), kOffsets.data(), 4, d);
  CHECK(d.size() == 2 && d.scans() == 1 && d.beams == kScan3Of4 && (d.scan == VecU{0, 0}));
  CHECK((d.sent == VecU{JobBatch::kUnseen, JobBatch::kUnseen, JobBatch::kUnseen, 0}));
}

static void check_dealing()
{
  JobBatch b;
  collect_job_batch(4, kJobs.data(), kJobScan.data(), 5, kPoints.data(), kOffsets.data(), 4, b);
  // the search's records: the batch's 4 in front of 5 rows, moved in place from the last -- job 1,
  // the empty scan's, in the middle keeps what lay there
  VecD records = {10.0, 11.0, 20.0, 21.0, 30.0, 31.0, 40.0, 41.0, 0.0, 0.0};
  move_match_records(b, 2, records.data());
  CHECK((records == VecD{10.0, 11.0, 20.0, 21.0, 20.0, 21.0, 30.0, 31.0, 40.0, 41.0}));
  // all jobs in the batch: nothing moves
  JobBatch whole;
  const VecU same = {0, 0, 2, 0, 3};
  collect_job_batch(4, kJobs.data(), same.data(), 5, kPoints.data(), kOffsets.data(), 4, whole);
  VecD five = {1.0, 2.0, 3.0, 4.0, 5.0};
  move_match_records(whole, 1, five.data());
  CHECK((five == VecD{1.0, 2.0, 3.0, 4.0, 5.0}));
  // the lattice scores: rows of 3, jobs 1 (not in the batch) and 3 (marked: its sequential call writes them) untouched
  const VecD batch_scores = {0.0, 0.1, 0.2, 2.0, 2.1, 2.2, 3.0, 3.1, 3.2, 4.0, 4.1, 4.2};
  VecD scores(15, -1.0);
  deal_lattice_scores(b, batch_scores.data(), 3, {0, 1, 0, 1, 0}, scores.data());
  CHECK((scores == VecD{0.0, 0.1, 0.2, -1.0, -1.0, -1.0, 2.0, 2.1, 2.2, -1.0, -1.0, -1.0, 4.0, 4.1, 4.2}));

  // the registration's records: {pose, f0, f, g, H upper, evals, steps, status, 0}; the sums over N beams -> / N
  VecD rec(4 * 18, 0.0);
  const double n_of[4] = {4.0, 3.0, 4.0, 4.0};
  for (size_t j = 0; j < 4; ++j)
  {
    double * r = rec.data() + 18 * j;
    r[0] = 100.0 + j, r[1] = 200.0 + j, r[2] = 300.0 + j;
    r[3] = -12.0 * n_of[j], r[4] = -24.0 * n_of[j];
    for (int d = 0; d < 3; ++d) r[5 + d] = (d + 1.0) * n_of[j];
    for (int d = 0; d < 6; ++d) r[8 + d] = (10.0 + d) * n_of[j];
    r[14] = 5.0 + j, r[15] = 3.0 + j, r[16] = static_cast<double>(j % 3);
  }
  VecD poses(15, -1.0), scores5(5, -1.0), starts(5, -1.0), grads(15, -1.0), hess(45, -1.0);
  std::vector<int32_t> status(5, 77);
  VecU evals(10, 77u);
  deal_refine_records(b, rec.data(), 18, RefineOut{poses.data(), scores5.data(), starts.data(), grads.data(), hess.data(), status.data(), evals.data()});
  CHECK((poses == VecD{100.0, 200.0, 300.0, -1.0, -1.0, -1.0, 101.0, 201.0, 301.0, 102.0, 202.0, 302.0, 103.0, 203.0, 303.0}));
  CHECK((scores5 == VecD{-24.0, -1.0, -24.0, -24.0, -24.0}) && (starts == VecD{-12.0, -1.0, -12.0, -12.0, -12.0}));
  CHECK((status == std::vector<int32_t>{0, 77, 1, 2, 0}));
  CHECK((evals == VecU{5, 3, 77, 77, 6, 4, 7, 5, 8, 6}));
  const VecD H = {10.0, 11.0, 12.0, 11.0, 13.0, 14.0, 12.0, 14.0, 15.0};   // xx xy xt / xy yy yt / xt yt tt
  for (size_t k = 0; k < 5; ++k)
  {
    const VecD g(grads.begin() + 3 * k, grads.begin() + 3 * k + 3), h(hess.begin() + 9 * k, hess.begin() + 9 * k + 9);
    CHECK(k == 1 ? (g == VecD{-1.0, -1.0, -1.0}) : (g == VecD{1.0, 2.0, 3.0}));
    CHECK(k == 1 ? h == VecD(9, -1.0) : h == H);
  }
  // the optional outputs may be absent
  deal_refine_records(b, rec.data(), 18, RefineOut{poses.data(), scores5.data(), nullptr, nullptr, nullptr, status.data(), nullptr});

  // the verification's records
  const VecU vrec = {1, 2, 3, 4, 5, 6, 7, 8};
  VecU vout(10, 0u);
  deal_verify_records(b, vrec.data(), 2, vout.data());
  CHECK((vout == VecU{1, 2, 0, 0, 3, 4, 5, 6, 7, 8}));
}

static void check_refusals()
{
  const std::string who = "w";
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const auto list = [&](const VecD & jobs, const VecU * job_scan, const double * points, const VecZ & offsets) {
    return job_list_refusal(who, jobs.data(), job_scan != nullptr ? job_scan->data() : nullptr, jobs.size() / 3, points, offsets.data(),
                            offsets.size() - 1);
  };
  // the list as it is: taken
  CHECK(job_list_size_refusal(who, 5, 4).empty() && job_list_size_refusal(who, 1u << 20, 1u << 20).empty());
  CHECK(list(kJobs, &kJobScan, kPoints.data(), kOffsets).empty());
  // each refusal, its text
  CHECK(job_list_size_refusal(who, (1u << 20) + 1, 4) == "w: too many jobs or scans");
  CHECK(job_list_size_refusal("match_scans", 5, (1u << 20) + 1) == "match_scans: too many jobs or scans");
  CHECK(list(kJobs, nullptr, kPoints.data(), kOffsets) == "w: no job_scan (job k uses scan k): n_scans must equal n_jobs");
  const VecZ decreasing = {0, 6, 6, 5, 18};
  CHECK(list(kJobs, &kJobScan, kPoints.data(), decreasing) == "w: scan 2: point_offsets decrease");
  CHECK(list(kJobs, &kJobScan, nullptr, kOffsets) == "w: null input");
  CHECK(list(kJobs, &kJobScan, nullptr, VecZ{3, 3, 3, 3, 3}).empty());   // (no points at all: none are read)
  VecD bad_pose = kJobs;
  bad_pose[3 * 3 + 2] = nan;
  CHECK(list(bad_pose, &kJobScan, kPoints.data(), kOffsets) == "w: job 3: the pose is not finite");
  bad_pose = kJobs;
  bad_pose[1] = -inf;
  CHECK(list(bad_pose, &kJobScan, kPoints.data(), kOffsets) == "w: job 0: the pose is not finite");
  const VecU bad_scan = {0, 7, 2, 0, 3};
  CHECK(list(kJobs, &bad_scan, kPoints.data(), kOffsets) == "w: job 1: scan 7 of 4");
  // two at once: which one is given
  CHECK(list(kJobs, nullptr, nullptr, decreasing) == "w: no job_scan (job k uses scan k): n_scans must equal n_jobs");
  bad_pose = kJobs;
  bad_pose[0] = nan;
  CHECK(list(bad_pose, &bad_scan, nullptr, decreasing) == "w: scan 2: point_offsets decrease");
  CHECK(list(bad_pose, &bad_scan, nullptr, kOffsets) == "w: null input");
  CHECK(list(bad_pose, &bad_scan, kPoints.data(), kOffsets) == "w: job 0: the pose is not finite");
  bad_pose = kJobs;
  bad_pose[3 * 3] = nan;
  CHECK(list(bad_pose, &bad_scan, kPoints.data(), kOffsets) == "w: job 1: scan 7 of 4");       // the earlier job
  const VecU bad_scan_3 = {0, 1, 2, 9, 3};
  CHECK(list(bad_pose, &bad_scan_3, kPoints.data(), kOffsets) == "w: job 3: the pose is not finite");   // of one job: its pose first
}

int main()
{
  check_collection();
  check_dealing();
  check_refusals();
  if (failures == 0) std::printf("OK\n");
  return failures == 0 ? 0 : 1;
}
