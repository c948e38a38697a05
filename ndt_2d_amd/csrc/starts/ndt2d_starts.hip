// Batched match from K start poses: ONE scan against the grid INSTALLED in the context, a full
// matchScan lattice around each of K starts, in one upload, one search launch, one reduction
// launch and one read-back per chunk (gfx950 / MI355X).
//
// Reference: a node that loads its map (src/ndt_mapper.cpp:106-116,155-186) refuses every scan
// until somebody posts `initialpose` (:315-320).  The remedy with this library -- matchScan
// (src/scan_matcher_ndt.cpp:76-150) from every graph node's pose under a few headings, keep the
// best response -- is K sequential searches, each one launch and one host round trip, each a
// lattice that fills a fraction of the chip.  The K searches are independent and read the same
// map.
//
// This is the batched scan tracking (../scans/ndt2d_scans.hip: K (scan, pose) jobs) with one scan
// that every job names, and its host engine runs it: the entry points here check their arguments
// and hand the call to match_jobs (../batch/ndt2d_batch_host.h) with n_scans = 1 and one_scan
// set, which makes the blocks take StartSlots -- a 24-byte record per start, no order table, the
// call's beams -- where a job's block takes JobSlots.  The kernels
// (../batch/ndt2d_batch_search.h), the upload, the chunking, the bits of a raw score and what
// happens off the grid are described there; with one beam count there is one launch per chunk:
// K x n_theta blocks, 1,280 of seven waves for the plugin's defaults and K = 16, where one
// sequential search is 80 x 7 tiles.  A start off the map scores 0.0 everywhere: no winner.
//
// The object is a type of its own with its own engine state, so timing set on it does not show
// on a matcher's ndt2d_scans object, nor the other way round.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
// (nothing is launched from here: ndt2d_batch_host.h brings JobsEngine and match_jobs, and with
// them the kernel header, whose reduce kernel this unit compiles without using it)
#include "batch/ndt2d_batch_search.h"
#include "batch/ndt2d_batch_host.h"

struct ndt2d_starts : ndt2d::JobsEngine
{
};

using ndt2d::batch_fail;

extern "C" {

int ndt2d_starts_create(ndt2d_handle h, size_t max_starts, ndt2d_starts ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || max_starts == 0 || max_starts > 4096) return NDT2D_ERR_INVALID;
  ndt2d_starts * s = new ndt2d_starts();
  s->h = h;
  s->device = ndt2d_device_id(h);
  s->max_jobs = max_starts;
  *out = s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_starts_destroy(ndt2d_starts * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::batch_drain(s);
  ndt2d::batch_release(s);
  delete s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_starts_last_error(ndt2d_starts * s)
{
  return s != nullptr ? s->err.c_str() : "null starts";
}

int ndt2d_starts_set_timing(ndt2d_starts * s, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(s, enabled);
  NDT2D_C_CATCH(s)
}

int ndt2d_starts_last_ms(ndt2d_starts * s, float * search_ms, float * reduce_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(s, "starts", search_ms, reduce_ms);
  NDT2D_C_CATCH(s)
}

int ndt2d_starts_match(ndt2d_starts * s, const double * starts_xyt, size_t n_starts, const double * beams_xy,
                       size_t n_beams, const double * dth, size_t n_th, const double * dlin, size_t n_lin,
                       double * records_out, double * all_scores)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_starts == 0) return NDT2D_OK;
  if (starts_xyt == nullptr || records_out == nullptr || beams_xy == nullptr || dth == nullptr || dlin == nullptr)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: null argument");
  }
  // what ndt2d_set_beams / ndt2d_set_search refuse
  if (n_beams == 0 || n_beams > (1u << 20)) return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: bad argument (n_beams)");
  if (n_th == 0 || n_lin == 0 || n_th > (1u << 24) || n_lin > 46340)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: bad argument (lattice)");
  }
  if (n_starts >= (1u << 24)) return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: bad argument (n_starts)");
  // every start is checked before anything is launched
  for (size_t k = 0; k < n_starts; ++k)
  {
    if (!std::isfinite(starts_xyt[3 * k]) || !std::isfinite(starts_xyt[3 * k + 1]) || !std::isfinite(starts_xyt[3 * k + 2]))
    {
      return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_starts_match: start " + std::to_string(k) + ": the pose is not finite");
    }
  }
  const size_t beam_offsets[2] = {0, n_beams};
  const ndt2d::JobsCall t{{starts_xyt, nullptr, n_starts, beams_xy, beam_offsets, 1}, true, dth, n_th, dlin, n_lin};
  return ndt2d::match_jobs(s, "ndt2d_starts_match", t, records_out, all_scores);
  NDT2D_C_CATCH(s)
}

}  // extern "C"
