// The (scan, pose) job list every batched call takes, on the host: K jobs over S scans, each scan's
// beams once however many jobs name it.  The searches (scans/ndt2d_scans.hip, with starts/ through
// its engine), the Newton registrations (refine/ndt2d_refine.hip: jobs on the installed grid;
// closure/ndt2d_closure.hip: jobs on the loop closure's candidate maps) and the verifications
// (verify/ndt2d_verify.hip and the closure's) share it: the list itself, what they refuse about
// scans and jobs -- one text, so that the objects cannot drift apart in what they refuse --, what
// the registrations refuse about their rules, and which scans a chunk uploads, with their copy
// into the stage.  Plain C++: no HIP.
#ifndef NDT2D_REFINE_JOBS_H_
#define NDT2D_REFINE_JOBS_H_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ndt2d
{

namespace refine_jobs
{

constexpr size_t kMaxScanBeams = size_t(1) << 20;   // what ndt2d_set_beams takes
constexpr uint64_t kNotSent = ~uint64_t(0);

// A call's jobs and scans.  The objects' own calls hold one beside what only they take.
struct JobList
{
  const double * jobs_xyt;
  const uint32_t * job_scan;   // NULL: job k uses scan k
  size_t n_jobs;
  const double * beams_xy;
  const size_t * beam_offsets;
  size_t n_scans;
  size_t scan_of(size_t k) const { return job_scan != nullptr ? job_scan[k] : k; }
  size_t beams_of(size_t k) const { return beam_offsets[scan_of(k) + 1] - beam_offsets[scan_of(k)]; }
};

// What a registration refuses about its rules: the refusal's text, prefixed with `entry`, or an
// empty string.
inline std::string rules_refusal(const char * entry, uint32_t max_evals, double tol_lin, double tol_ang)
{
  const std::string who = std::string(entry) + ": ";
  if (max_evals == 0) return who + "bad argument (max_evals == 0)";
  if (!(tol_lin >= 0.0) || !(tol_ang >= 0.0) || !std::isfinite(tol_lin) || !std::isfinite(tol_ang))
  {
    return who + "bad argument (a tolerance is negative or not finite)";
  }
  return std::string();
}

// Every scan and every job of a call, checked before anything is launched.  Returns the refusal's
// text, prefixed with `entry` (the message names the scan or the job), or an empty string.
// job_scan NULL: job k uses scan k.
inline std::string refusal(const char * entry, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                           const size_t * beam_offsets, size_t n_scans)
{
  const std::string who = std::string(entry) + ": ";
  if (n_jobs >= (1u << 24) || n_scans >= (1u << 24)) return who + "bad argument (n_jobs, n_scans)";
  if (job_scan == nullptr && n_scans != n_jobs)
  {
    return who + "bad argument (no job_scan: job k uses scan k, n_scans must equal n_jobs)";
  }
  for (size_t sc = 0; sc < n_scans; ++sc)
  {
    if (beam_offsets[sc + 1] < beam_offsets[sc]) return who + "scan " + std::to_string(sc) + ": beam_offsets decrease";
    const size_t count = beam_offsets[sc + 1] - beam_offsets[sc];
    // (what ndt2d_set_beams refuses)
    if (count == 0 || count > kMaxScanBeams)
    {
      return who + "scan " + std::to_string(sc) + ": " + std::to_string(count) + " beams (1 .. 2^20)";
    }
  }
  for (size_t k = 0; k < n_jobs; ++k)
  {
    if (!std::isfinite(jobs_xyt[3 * k]) || !std::isfinite(jobs_xyt[3 * k + 1]) || !std::isfinite(jobs_xyt[3 * k + 2]))
    {
      return who + "job " + std::to_string(k) + ": the pose is not finite";
    }
    if (job_scan != nullptr && job_scan[k] >= n_scans)
    {
      return who + "job " + std::to_string(k) + ": scan " + std::to_string(job_scan[k]) + " of " + std::to_string(n_scans);
    }
  }
  return std::string();
}

// The rules, then the list: what a registration refuses, in that order.
inline std::string refusal(const char * entry, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                           const size_t * beam_offsets, size_t n_scans, uint32_t max_evals, double tol_lin, double tol_ang)
{
  const std::string rules = rules_refusal(entry, max_evals, tol_lin, tol_ang);
  return !rules.empty() ? rules : refusal(entry, jobs_xyt, job_scan, n_jobs, beam_offsets, n_scans);
}

// The scans a chunk's jobs name, each once, in the order the jobs first name them: scan_first[s] =
// the scan's first beam within the chunk's beams (kNotSent: not sent), sent = the scans in upload
// order.  jobs[0 .. n): the chunk's jobs, as indices into the call's; scan_of(k): job k's scan.
// Returns the chunk's beam count.
template <class JOB_AT, class SCAN_OF>
inline size_t plan_sent_scans(size_t n, JOB_AT job_at, SCAN_OF scan_of, const size_t * beam_offsets, size_t n_scans,
                              std::vector<uint64_t> & scan_first, std::vector<uint32_t> & sent)
{
  scan_first.assign(n_scans, kNotSent);
  sent.clear();
  size_t n_beams = 0;
  for (size_t b = 0; b < n; ++b)
  {
    const size_t sc = scan_of(job_at(b));
    if (scan_first[sc] == kNotSent)
    {
      scan_first[sc] = n_beams;
      sent.push_back(static_cast<uint32_t>(sc));
      n_beams += beam_offsets[sc + 1] - beam_offsets[sc];
    }
  }
  return n_beams;
}

// The beams of the sent scans into the chunk's beams (`to`, [beam][2]), each scan at its
// scan_first; beams_xy / beam_offsets: the call's.
inline void copy_sent_scans(const std::vector<uint32_t> & sent, const std::vector<uint64_t> & scan_first, const double * beams_xy,
                            const size_t * beam_offsets, double * to)
{
  for (const uint32_t sc : sent)
  {
    std::memcpy(to + 2 * scan_first[sc], beams_xy + 2 * beam_offsets[sc],
                2 * (beam_offsets[sc + 1] - beam_offsets[sc]) * sizeof(double));
  }
}

}  // namespace refine_jobs

}  // namespace ndt2d

#endif  // NDT2D_REFINE_JOBS_H_
