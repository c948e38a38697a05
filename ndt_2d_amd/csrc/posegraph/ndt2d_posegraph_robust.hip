// The robust losses of the pose graph on the host (include/ndt2d_hip.h, "Robust losses"): a loss's
// values for a caller, and the object's loss, its scale and the constraints it applies to.  Nothing
// is launched from here: the setters leave the object marked, and the next evaluate, solve or
// marginals call sends what changed (pg_send_loss, posegraph/ndt2d_posegraph.hip) and takes the
// kernels of the loss in force.  The losses themselves are posegraph/ndt2d_posegraph_loss.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "posegraph/ndt2d_posegraph_loss.h"
#include "posegraph/ndt2d_posegraph_state.h"

using ndt2d::batch_fail;

extern "C" {

int ndt2d_robust_rho(const char * kind, double scale, double s, double * rho3_out)
{
  NDT2D_C_TRY
  const int loss = ndt2d::pg_loss_kind(kind);
  if (rho3_out == nullptr || loss < 0 || !(scale > 0.0) || !std::isfinite(scale) || !(s >= 0.0) || !std::isfinite(s)) return NDT2D_ERR_INVALID;
  return ndt2d::posegraph::loss_evaluate(loss, scale, s, rho3_out) ? NDT2D_OK : NDT2D_ERR_INVALID;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_robust_set_loss(ndt2d_posegraph * s, const char * kind, double scale)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const int loss = ndt2d::pg_loss_kind(kind);
  if (loss < 0)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, std::string("ndt2d_robust_set_loss: \"") + (kind != nullptr ? kind : "") +
                                              "\" (\"trivial\", \"huber\" or \"cauchy\")");
  }
  if (loss != ndt2d::posegraph::kLossTrivial)
  {
    if (!(scale > 0.0) || !std::isfinite(scale)) return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_robust_set_loss: the scale is not finite and > 0");
    if (scale != s->loss_scale) s->loss_sent = false;
    s->loss_scale = scale;
  }
  s->loss = loss;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

const char * ndt2d_robust_loss(ndt2d_posegraph * s, double * scale_out)
{
  if (s != nullptr && scale_out != nullptr) *scale_out = s->loss_scale;
  return s == nullptr ? "" : ndt2d::kPgLossNames[s->loss];
}

int ndt2d_robust_select(ndt2d_posegraph * s, const uint8_t * robust, size_t m)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const int rc = ndt2d::pg_ready(s, "ndt2d_robust_select");
  if (rc != NDT2D_OK) return rc;
  if (robust == nullptr)
  {
    s->robust.clear();
  }
  else
  {
    if (m != s->m)
    {
      return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_robust_select: " + std::to_string(m) + " bytes, the graph has " + std::to_string(s->m) +
                                                " constraints");
    }
    s->robust.assign(robust, robust + m);
    if (m == 0) s->robust.clear();
  }
  s->loss_sent = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
