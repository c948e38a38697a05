// The (scan, pose) job list of the matcher's batched calls (match_scans, refine_scans, verify_scans,
// refine_candidates, verify_candidates: host/ndt2d_batched.cpp), between the caller's arrays and the
// device objects': what the calls refuse about such a list, the jobs and subsampled scans that go
// into the one device call (a scan once however many jobs name it; a scan without points and its
// jobs not at all), and the way back of the call's records to their jobs.  Plain C++: no HIP, and
// nothing of the matcher -- the refusals are texts, the caller fails with them.
#ifndef NDT2D_JOB_BATCH_H_
#define NDT2D_JOB_BATCH_H_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "host/ndt2d_host_ndt.h"

namespace ndt2d
{
namespace host
{

// "Every point" as subsample_into takes a limit: what the registrations and the verifications make
// of max_beams 0 (match_scans gives laser_max_beams as it is: 0 beams).
constexpr size_t kEveryPoint = ~size_t(0);

// What every call refuses first: the list's size.  The refusal's text, or an empty string.
inline std::string job_list_size_refusal(const std::string & who, size_t n_jobs, size_t n_scans)
{
  if (n_jobs > (1u << 20) || n_scans > (1u << 20)) return who + ": too many jobs or scans";
  return std::string();
}

// What every call refuses about the scans and the jobs of a list whose size it takes; job_scan
// NULL: job k uses scan k.  The refusal's text, or an empty string.
inline std::string job_list_refusal(const std::string & who, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                                    const double * points_xy, const size_t * point_offsets, size_t n_scans)
{
  if (job_scan == nullptr && n_scans != n_jobs) return who + ": no job_scan (job k uses scan k): n_scans must equal n_jobs";
  for (size_t sc = 0; sc < n_scans; ++sc)
  {
    if (point_offsets[sc + 1] < point_offsets[sc]) return who + ": scan " + std::to_string(sc) + ": point_offsets decrease";
  }
  if (n_scans > 0 && point_offsets[n_scans] > point_offsets[0] && points_xy == nullptr) return who + ": null input";
  for (size_t k = 0; k < n_jobs; ++k)
  {
    if (!std::isfinite(jobs_xyt[3 * k]) || !std::isfinite(jobs_xyt[3 * k + 1]) || !std::isfinite(jobs_xyt[3 * k + 2]))
    {
      return who + ": job " + std::to_string(k) + ": the pose is not finite";
    }
    if (job_scan != nullptr && job_scan[k] >= n_scans)
    {
      return who + ": job " + std::to_string(k) + ": scan " + std::to_string(job_scan[k]) + " of " + std::to_string(n_scans);
    }
  }
  return std::string();
}

// The jobs of a device call: every scan a job names as matchScan and scorePoints take it --
// subsampled beams (src/scan_matcher_ndt.cpp:95-96,110 and :165-166,171) --, once per scan, in the
// order the jobs first name them; a scan without beams is not among them, and neither are its jobs.
struct JobBatch
{
  static constexpr uint32_t kUnseen = ~0u, kEmpty = ~0u - 1u;
  std::vector<double> beams, xyt;    // [beam][2] of the scans sent; [job][3]
  std::vector<size_t> beam_offsets;  // [scans sent + 1]
  std::vector<uint32_t> job, scan;   // the jobs of the device call (ascending), and their scans among those sent
  std::vector<uint32_t> sent;        // scan of the list -> its index among the scans sent (or kUnseen, kEmpty)
  size_t size() const { return job.size(); }
  size_t scans() const { return beam_offsets.size() - 1; }
  size_t scan_beams(size_t s) const { return beam_offsets[s + 1] - beam_offsets[s]; }
  size_t beams_of(size_t j) const { return scan_beams(scan[j]); }   // of job j of the batch
};

// beam_limit: as subsample_into takes it (kEveryPoint: all).  A checked list (job_list_refusal).
inline void collect_job_batch(size_t beam_limit, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                              const double * points_xy, const size_t * point_offsets, size_t n_scans, JobBatch & b)
{
  b.sent.assign(n_scans, JobBatch::kUnseen);
  std::vector<double> one;
  b.beam_offsets.assign(1, 0);
  for (size_t k = 0; k < n_jobs; ++k)
  {
    const size_t sc = job_scan != nullptr ? static_cast<size_t>(job_scan[k]) : k;
    if (b.sent[sc] == JobBatch::kUnseen)
    {
      subsample_into(one, points_xy + 2 * point_offsets[sc], point_offsets[sc + 1] - point_offsets[sc], beam_limit);
      if (one.empty())
      {
        b.sent[sc] = JobBatch::kEmpty;
      }
      else
      {
        b.sent[sc] = static_cast<uint32_t>(b.scans());
        b.beams.insert(b.beams.end(), one.begin(), one.end());
        b.beam_offsets.push_back(b.beams.size() / 2);
      }
    }
    if (b.sent[sc] == JobBatch::kEmpty) continue;
    b.job.push_back(static_cast<uint32_t>(k));
    b.scan.push_back(b.sent[sc]);
    b.xyt.insert(b.xyt.end(), jobs_xyt + 3 * k, jobs_xyt + 3 * k + 3);
  }
}

// The beams of the batch's jobs, job after job (a shared scan counts once per job).
inline size_t batch_beams(const JobBatch & b)
{
  size_t n = 0;
  for (size_t j = 0; j < b.size(); ++j) n += b.beams_of(j);
  return n;
}

// Where each job's beams start in a verification's per-beam arrays ([n_jobs + 1]): the batch's jobs
// in order, the jobs of scans without points between them with no beams.
inline void fill_verify_offsets(const JobBatch & b, size_t n_jobs, size_t * beam_offsets_out)
{
  size_t at = 0, j = 0;
  for (size_t k = 0; k < n_jobs; ++k)
  {
    beam_offsets_out[k] = at;
    if (j < b.size() && b.job[j] == k)
    {
      at += b.beams_of(j);
      ++j;
    }
  }
  beam_offsets_out[n_jobs] = at;
}

// A search's records ([batch job][rec] in front of a [job][rec] array) to their jobs' slots, in
// place.  From the last: b.job ascends, so record j's slot b.job[j] >= j holds no record still to be moved.
inline void move_match_records(const JobBatch & b, size_t rec, double * records)
{
  for (size_t j = b.size(); j-- > 0;)
  {
    const size_t k = b.job[j];
    if (k != j) std::memcpy(records + k * rec, records + j * rec, rec * sizeof(double));
  }
}

// A search's lattice scores ([batch job][n_lattice]) into the rows of their jobs, but for the jobs
// marked in `skip`.
inline void deal_lattice_scores(const JobBatch & b, const double * batch_scores, size_t n_lattice, const std::vector<char> & skip,
                                double * scores_out)
{
  for (size_t j = 0; j < b.size(); ++j)
  {
    const size_t k = b.job[j];
    if (!skip[k]) std::memcpy(scores_out + k * n_lattice, batch_scores + j * n_lattice, n_lattice * sizeof(double));
  }
}

// The outputs of a Newton registration (refine_scans, refine_candidates); all but poses, scores and
// status are optional.
struct RefineOut
{
  double * poses, * scores, * start_scores, * gradients, * hessians;
  int32_t * status;
  uint32_t * evals;
};

// A registration's records ([batch job][rec_doubles = 18]: pose, f0, f, g, H (upper), evals, steps,
// status) into the outputs of their jobs.
inline void deal_refine_records(const JobBatch & b, const double * records, size_t rec_doubles, const RefineOut & o)
{
  for (size_t j = 0; j < b.size(); ++j)
  {
    const size_t k = b.job[j];
    const double * rec = records + j * rec_doubles;
    // f, g, H of the sum over the scan's N beams -> of `score / N` (:177)
    const double n = static_cast<double>(b.beams_of(j));
    std::memcpy(o.poses + 3 * k, rec, 3 * sizeof(double));
    o.scores[k] = rec[4] / n;
    o.status[k] = static_cast<int32_t>(rec[16]);
    if (o.start_scores != nullptr) o.start_scores[k] = rec[3] / n;
    if (o.gradients != nullptr)
    {
      for (int d = 0; d < 3; ++d) o.gradients[3 * k + d] = rec[5 + d] / n;
    }
    if (o.hessians != nullptr)
    {
      double * h = o.hessians + 9 * k;
      h[0] = rec[8] / n;
      h[1] = h[3] = rec[9] / n;
      h[2] = h[6] = rec[10] / n;
      h[4] = rec[11] / n;
      h[5] = h[7] = rec[12] / n;
      h[8] = rec[13] / n;
    }
    if (o.evals != nullptr)
    {
      o.evals[2 * k] = static_cast<uint32_t>(rec[14]);
      o.evals[2 * k + 1] = static_cast<uint32_t>(rec[15]);
    }
  }
}

// A verification's records ([batch job][rec_u32]) into the rows of their jobs.
inline void deal_verify_records(const JobBatch & b, const uint32_t * records, size_t rec_u32, uint32_t * records_out)
{
  for (size_t j = 0; j < b.size(); ++j)
  {
    std::memcpy(records_out + static_cast<size_t>(b.job[j]) * rec_u32, records + j * rec_u32, rec_u32 * sizeof(uint32_t));
  }
}

}  // namespace host
}  // namespace ndt2d

#endif  // NDT2D_JOB_BATCH_H_
