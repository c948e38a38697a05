/*
 * ndt2d_hip.h -- C-ABI of libndt2d_hip.so: hand-written HIP (gfx950 / MI355X)
 * kernels for ndt_2d's NDT scan-matching hot path, plus the host-side mirror of
 * the reference's ndt_2d::ScanMatcher plugin interface for that path.
 *
 * Plain C, no torch / Eigen / ROS types: pointers, sizes, doubles.  Every entry
 * point returns an int status (NDT2D_OK == 0) and never throws.  Citations are
 * file:line in the reference repository (mikeferguson/ndt_2d @ 2024-12-18).
 *
 * Two layers live in the one library:
 *
 *  (1) device layer  ndt2d_*         one opaque context per GPU and per plugin
 *      instance: resident NDT grid, resident beams, search tables, kernel
 *      launches.  This is what a cgo/JNI/ctypes/pluginlib binding calls.
 *
 *  (2) matcher layer ndt2d_matcher_* the reference's ScanMatcherNDT object
 *      (initialize / addScans / matchScan / scoreScan / scorePoints / reset,
 *      include/ndt_2d/scan_matcher.hpp:42-91) restated over layer (1), plus the
 *      additive batched particle path (ParticleFilter::measure,
 *      src/particle_filter.cpp:78-89).  The pluginlib shim
 *      (ndt_2d_amd/plugin/scan_matcher_ndt_hip.cpp) is a thin wrapper of it.
 *
 * There is NO CPU fallback: nothing in this library exists without a usable GPU
 * (ndt2d_create / ndt2d_matcher_create return NDT2D_ERR_NO_DEVICE / NDT2D_ERR_HIP),
 * and every search, every batch of poses and every scan of more than 256 beams is
 * evaluated on the GPU.  What runs on the HOST, by design and on a live matcher only
 * (DESIGN.md 3.6): ONE pose of a short scan -- ndt2d_matcher_score_points /
 * _score_scan as the unchanged ParticleFilter::measure calls them, once per particle
 * (src/particle_filter.cpp:81-87) -- is scored by the calling thread from the host
 * copy of the NDT in the reference's order (0.4 us instead of a 9 us launch + PCIe
 * round trip; ndt2d_matcher_set_single_pose_path(m, "device", 0) turns it off), and
 * the few candidates of a marked near-tie are rescored in the reference's arithmetic.
 */
#ifndef NDT2D_HIP_H_
#define NDT2D_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDT2D_OK 0
#define NDT2D_ERR_INVALID 1    /* bad argument (NULL, zero size, bad range) */
#define NDT2D_ERR_NO_GRID 2    /* compute call before ndt2d_set_grid / addScans */
#define NDT2D_ERR_HIP 3        /* a HIP runtime call failed; see ndt2d_last_error */
#define NDT2D_ERR_NO_DEVICE 4  /* no GPU visible to this process */
#define NDT2D_ERR_STATE 5      /* call sequence error (e.g. fetch before launch) */
#define NDT2D_ERR_ALLOC 6      /* host memory could not be had (std::bad_alloc caught at the boundary) */
#define NDT2D_ERR_INTERNAL 7   /* any other C++ exception caught at the boundary; see ndt2d_last_error */

#define NDT2D_NO_INDEX UINT64_MAX

/* ------------------------------------------------------------------------ */
/* (1) device layer                                                         */
/* ------------------------------------------------------------------------ */

typedef struct ndt2d_context * ndt2d_handle;

/* ABI version of this header: bumped whenever an export is added, a signature changes or a
 * default changes results.  4 (round 6): + NDT2D_ERR_ALLOC / NDT2D_ERR_INTERNAL,
 * ndt2d_host_build_grid_ex, and the round-5 additions that had gone out under 3 (pose_sums_*,
 * pf_finalize_totals_launch, pipeline_pieces, multi_thresholds, eigenvalue_form, build_info).  A
 * consumer compares ndt2d_abi_version() with the NDT2D_ABI_VERSION it was compiled against
 * (the pluginlib shim does, in initialize). */
#define NDT2D_ABI_VERSION 4
int ndt2d_abi_version(void);
/* Which sources this library was compiled from: "NDT2D_SOURCE_SHA256=<64 hex digits> arch=...
 * compiler=...".  The hash is ndt_2d_amd/build.py's source_sha256() (csrc/ *.hip, *.cpp, *.h,
 * this header, the compiler flags) at build time: the tests, bench.py and tests/conftest.py
 * compare it with the tree they run from, so a stale binary cannot stand in for the sources. */
const char * ndt2d_build_info(void);

/* One context per (plugin instance, GPU).  The reference keeps all state per
 * ScanMatcherNDT instance (std::unique_ptr<NDT> ndt_,
 * include/ndt_2d/scan_matcher_ndt.hpp:102) and runs two instances concurrently
 * on two threads (src/ndt_mapper.cpp:141-142,508-515,634-643): a context owns
 * its own HIP stream and buffers and holds no process-global mutable state. */
int ndt2d_create(ndt2d_handle * out, int device_id);
int ndt2d_destroy(ndt2d_handle h);
/* Message of the last failure on this context ("" if none).  Never NULL. */
const char * ndt2d_last_error(ndt2d_handle h);
/* Launch on a caller-owned hipStream_t instead of the context's own stream
 * (NULL restores the own stream).  ndt2d_get_stream returns the active one. */
int ndt2d_set_stream(ndt2d_handle h, void * hip_stream);
void * ndt2d_get_stream(ndt2d_handle h);
int ndt2d_device_id(ndt2d_handle h);

/* Upload the NDT cell grid; replaces the NDT object built by
 * ScanMatcherNDT::addScans (src/scan_matcher_ndt.cpp:66-73).
 * cells6[i] = {mean_x, mean_y, information(0,0), information(0,1),
 * information(1,1), n} for cell i = grid_y * size_x + grid_x, i.e. the fields
 * Cell::score reads (src/ndt_model.cpp:105-116); size/origin/cell_size are
 * NDT::size_x_, size_y_, origin_x_, origin_y_, cell_size_
 * (include/ndt_2d/ndt_model.hpp:128-131). */
int ndt2d_set_grid(ndt2d_handle h, const double * cells6, uint32_t size_x, uint32_t size_y,
                   double cell_size, double origin_x, double origin_y);

/* The same grid given as the LIST of its cells that received points: cells6[k] (layout as
 * above) belongs to cell cell_index[k] = grid_y * size_x + grid_x, every cell not listed is
 * an empty one (n = 0, as NDT::NDT leaves it, src/ndt_model.cpp:118-126); a cell may be
 * listed once, in any order (a cell with n >= 5 listed twice: NDT2D_ERR_INVALID).  The mapper
 * rebuilds its local NDT for every scan (src/ndt_mapper.cpp:508-509); with a real lidar
 * that grid has tens of thousands of cells (scan poses +- range_max,
 * src/scan_matcher_ndt.cpp:52-66) of which the scans touch a thousand or two: the cost of
 * this call follows the list, not the grid. */
int ndt2d_set_grid_sparse(ndt2d_handle h, const uint32_t * cell_index, const double * cells6,
                          size_t n_listed, uint32_t size_x, uint32_t size_y, double cell_size,
                          double origin_x, double origin_y);

/* The same in two steps, for a host that can write its list straight into the library's pinned
 * staging buffer (no intermediate copy): begin hands out room for up to `capacity` listed cells
 * (cell_index_out[k], cells6_out[6 k .. 6 k + 5]), commit installs the first n_listed of them.
 * Nothing else may be called on the context in between. */
int ndt2d_grid_stage_begin(ndt2d_handle h, uint32_t size_x, uint32_t size_y, size_t capacity,
                           uint32_t ** cell_index_out, double ** cells6_out);
int ndt2d_grid_stage_commit(ndt2d_handle h, size_t n_listed, double cell_size, double origin_x,
                            double origin_y);

/* Build the NDT on the device from the scans themselves and install it: the
 * whole of ScanMatcherNDT::addScans (src/scan_matcher_ndt.cpp:49-74) --
 * bounding box of the scan poses +- range_max, NDT::addScan for every scan in
 * order (src/ndt_model.cpp:132-152), NDT::compute (:154-160).  Scan k has pose
 * poses_xyt[3k..3k+2] and robot-frame points points_xy[2*offsets[k] ..
 * 2*offsets[k+1]).  Every cell sees its points in the reference's order (stable
 * sort by cell), so the result is bit-identical to the host build.  Asynchronous
 * on the context's stream. */
int ndt2d_build_grid(ndt2d_handle h, double ndt_resolution, double range_max,
                     const double * poses_xyt, const double * points_xy, const size_t * offsets,
                     size_t n_scans);
/* ---- the fused small-map build and resident scans (csrc/build_small/) ----
 *
 * ndt2d_build_grid for a mapper-size map -- at most ndt2d_build_small_max_points() points
 * (16,384) on a grid of fewer than 65,535 cells -- with everything order-dependent in ONE
 * workgroup: the points are keyed, sorted by cell and walked in the reference's order in a
 * single launch that leaves the list of touched cells where ndt2d_grid_stage_begin / _commit
 * take it, so the build is three launches and one small read-back instead of a dozen stream
 * operations, and no host arithmetic.  Arguments, semantics and the grid (bit for bit) are
 * those of ndt2d_build_grid; the call returns when the grid is installed.  A map beyond the
 * limits: NDT2D_ERR_INVALID, ndt2d_build_small_last_error(h) names them, and the context is
 * left without a grid.
 *
 * The build lives beside the context and reaches it through this boundary only, so
 *  - its eigenvalue form is its own: ndt2d_build_small_set_eigenvalue_form(h, "eigen" |
 *    "closed") (ndt2d_set_eigenvalue_form does not reach it; the matcher layer sets both);
 *  - its messages are read with ndt2d_build_small_last_error(h);
 *  - the device memory it keeps for h (found by the handle) is freed by
 *    ndt2d_build_small_release(h), to be called before ndt2d_destroy(h) by a caller that used
 *    ndt2d_build_grid_small or the form setter on h (the matcher layer does).
 * ndt2d_build_grid_small_fits: 1 if a map of n_points points with these scan poses is within
 * the limits, 0 otherwise (or on a bad argument); it needs no context. */
int ndt2d_build_grid_small(ndt2d_handle h, double ndt_resolution, double range_max,
                           const double * poses_xyt, const double * points_xy, const size_t * offsets,
                           size_t n_scans);
int ndt2d_build_grid_small_fits(double ndt_resolution, double range_max, const double * poses_xyt,
                                size_t n_scans, size_t n_points);
size_t ndt2d_build_small_max_points(void);
int ndt2d_build_small_set_eigenvalue_form(ndt2d_handle h, const char * form);
const char * ndt2d_build_small_last_error(ndt2d_handle h);
int ndt2d_build_small_release(ndt2d_handle h);

/* Resident scans.  The mapper rebuilds its local NDT before every scan match from the last ten
 * scans (src/ndt_mapper.cpp:508-509) and the loop-closure thread does so for every candidate
 * (:634-635): nine of ten scans were on the device the cycle before, only the poses are new.
 * A scan store keeps the robot-frame points of the scans appended to it in device memory
 * (ids count from 0 in append order) and builds a map from any of them in any order through
 * the fused build above: per build only the poses and the {offset, count} table of the named
 * scans are uploaded.  It is an object of its own beside the context: it launches on the
 * context's current stream, installs the grid into that context, and must be destroyed before
 * ndt2d_destroy(h).
 *   append   copies n_points points (zero is allowed); the caller's buffer is free on return.
 *            A store that holds capacity_scans scans, or too few free points: NDT2D_ERR_INVALID,
 *            nothing is stored.
 *   reset    forgets every scan (ids start from 0 again); the installed grid stays.
 *   build    ScanMatcherNDT::addScans of the scans ids[0..n_scans) in that order with the poses
 *            poses_xyt[3k..3k+2]: the grid ndt2d_build_grid gives for the same scans and poses.
 *            An unknown id, a non-finite pose, a degenerate extent or a map beyond the fused
 *            build's limits: NDT2D_ERR_INVALID before anything is launched; the installed grid
 *            is left as it was.
 *   set_eigenvalue_form   "eigen" (default) or "closed", as ndt2d_set_eigenvalue_form. */
typedef struct ndt2d_scanstore ndt2d_scanstore;
int ndt2d_scanstore_create(ndt2d_handle h, size_t capacity_points, size_t capacity_scans,
                           ndt2d_scanstore ** out);
int ndt2d_scanstore_destroy(ndt2d_scanstore * store);
const char * ndt2d_scanstore_last_error(ndt2d_scanstore * store);
int ndt2d_scanstore_set_eigenvalue_form(ndt2d_scanstore * store, const char * form);
int ndt2d_scanstore_append(ndt2d_scanstore * store, const double * points_xy, size_t n_points,
                           size_t * id_out);
int ndt2d_scanstore_count(ndt2d_scanstore * store, size_t * n_scans_out);
int ndt2d_scanstore_reset(ndt2d_scanstore * store);
int ndt2d_scanstore_build(ndt2d_scanstore * store, const size_t * ids, const double * poses_xyt,
                          size_t n_scans, double ndt_resolution, double range_max);

/* ---- batched loop-closure match (csrc/closure/) ----
 *
 * The loop-closure thread matches every new scan against up to global_search_limit_ candidate
 * maps, each built from one or two old scans: reset(), addScans(begin, end), matchScan(scan)
 * per candidate (src/ndt_mapper.cpp:619-671).  ndt2d_closure_match does that for K candidates
 * in one build launch (a workgroup of the fused small-map build per candidate map, which also
 * writes the packed records and the cell -> record table the search reads), one search launch
 * over (candidate map x lattice) and one reduction, and reads all K records back in one copy.
 * An object of its own beside the context: it reads its scans from `store` (a store of the same
 * context), launches on the context's current stream, installs nothing into the context, and
 * must be destroyed before the store and before ndt2d_destroy(h).
 *
 *   create   max_candidates (1 .. 4,096): candidate maps of one launch; a call with more is
 *            processed in chunks of that many inside the call.
 *   match    candidate k is built from the stored scans ids[cand_offsets[k] .. cand_offsets[k + 1])
 *            in that order with the poses poses_xyt[3 j ..] (flat, parallel to ids): the grid
 *            ndt2d_scanstore_build gives for them with ndt_resolution / range_max.  The search
 *            is the one ndt2d_set_search_beams + ndt2d_match_launch(0, n_th) would run on that
 *            grid -- the same arguments: subsampled robot-frame beams, the scan pose, the
 *            visited offsets, host-libm cos / sin per theta step -- and every candidate starts
 *            from the same pose.  records_out[K][NDT2D_MATCH_RECORD_DOUBLES] receives
 *            {best_score, best_index (-1: none; + 0.5: near tie), acc[10]} per candidate,
 *            all_scores (optional) [K][n_th * n_lin * n_lin] every lattice candidate's raw score.
 *            A raw score has the bits of the small-lattice search's (the mapping every
 *            loop-closure-size lattice takes: ndt2d_set_variant); two calls give the same bits.
 *            A candidate with an unknown id, a non-finite pose, no scans, a degenerate extent
 *            or a map beyond the fused build's limits (ndt2d_build_grid_small_fits):
 *            NDT2D_ERR_INVALID before anything is launched, the message names the candidate.
 *            A candidate whose scans hold no points is a map without cells: every score 0.
 *   set_timing / last_ms   HIP events around the build and the search launch of the last
 *            (chunk of a) match, off by default. */
typedef struct ndt2d_closure ndt2d_closure;
int ndt2d_closure_create(ndt2d_handle h, ndt2d_scanstore * store, size_t max_candidates,
                         ndt2d_closure ** out);
int ndt2d_closure_destroy(ndt2d_closure * closure);
const char * ndt2d_closure_last_error(ndt2d_closure * closure);
int ndt2d_closure_match(ndt2d_closure * closure, size_t n_candidates, const size_t * cand_offsets,
                        const size_t * ids, const double * poses_xyt, double ndt_resolution,
                        double range_max, const double * beams_xy, size_t n_beams, double pose_x,
                        double pose_y, const double * dth, const double * cos_th,
                        const double * sin_th, size_t n_th, const double * dlin, size_t n_lin,
                        double * records_out, double * all_scores);
int ndt2d_closure_set_timing(ndt2d_closure * closure, int enabled);
int ndt2d_closure_last_ms(ndt2d_closure * closure, float * build_ms, float * search_ms);

/* How ndt2d_build_grid forms the eigenvalues of Cell::compute (src/ndt_model.cpp:84-85,
 * Eigen::EigenSolver<Eigen::Matrix2d>): "eigen" (default) = Eigen 3.4.0's RealSchur /
 * EigenSolver transcribed operation by operation for a 2 x 2 input (csrc/ndt2d_eigen2.h: the
 * input scaled by its largest entry, the Givens rotation of the 2 x 2 block, the diagonal read
 * back); "closed" = the closed form (a + d) / 2 +- sqrt(((a - d) / 2)^2 + b^2) of rounds 1-4.
 * The two differ in the last ulps; the difference reaches a cell's information matrix only
 * through the clamp branch (:88-96). */
int ndt2d_set_eigenvalue_form(ndt2d_handle h, const char * form);
/* Geometry and (optionally) the cells6 records of the installed grid, copied
 * back from the device.  Any output may be NULL. */
int ndt2d_get_grid(ndt2d_handle h, double * cells6_out, size_t capacity_cells, uint32_t * size_x,
                   uint32_t * size_y, double * cell_size, double * origin_x, double * origin_y);
/* ScanMatcherNDT::reset (src/scan_matcher_ndt.cpp:180-183). */
int ndt2d_clear_grid(ndt2d_handle h);
int ndt2d_has_grid(ndt2d_handle h);

/* What a kernel outside the context needs of the installed grid (csrc/starts/): the geometry of
 * NDT::getIndex and two device pointers -- cells_global[ncell + 1], one 64-byte line per cell
 * {mean_x, mean_y, h00, h01, h11, occ, 0, 0} with h = -0.5 * information, and occ_bits, bit i =
 * cell i can score (n >= 5); entry ncell of both stands for "off the grid".  Read-only, written
 * by every install path; valid until the next install or clear.  NDT2D_ERR_NO_GRID without a
 * grid. */
typedef struct ndt2d_grid_view
{
  const double * cells_global;
  const uint32_t * occ_bits;
  uint32_t size_x, size_y, ncell;
  int pow2;                 /* cell_size is a power of two: x * inv_cell_size == x / cell_size */
  double cell_size, inv_cell_size;
  double origin_x, origin_y;
} ndt2d_grid_view;
int ndt2d_grid_view_get(ndt2d_handle h, ndt2d_grid_view * out);

/* ---- batched match from K start poses (csrc/starts/) ----
 *
 * One scan, the grid INSTALLED in the context, K start poses, the full matchScan lattice around
 * each: what K calls of ndt2d_set_search_beams + ndt2d_match_launch(0, n_th) + ndt2d_match_fetch
 * give, in one upload, one search launch over (theta step x start), one reduction and one
 * read-back.  A node that loads a map and has no initial pose tries every graph node's pose under
 * a few headings that way (relocalisation); a tracker keeps several hypotheses alive.
 * An object of its own beside the context: it reads the grid installed at the time of the call
 * (any install path, any size or origin), installs nothing, launches on the context's current
 * stream, and must be destroyed before ndt2d_destroy(h).
 *
 *   create   max_starts (1 .. 4,096): starts of one launch; a call with more is processed in
 *            chunks inside the call.  Chunking changes no bit.
 *   match    starts_xyt[K][3]; beams_xy: the subsampled robot-frame beams; dth[n_th] / dlin[n_lin]:
 *            the visited offsets (ndt2d_set_search).  cos / sin of theta_k + dth[i] come from the
 *            host libm inside the call.  records_out[K][NDT2D_MATCH_RECORD_DOUBLES] receives
 *            {best_score, best_index (-1: none; + 0.5: near tie), acc[10]} per start, all_scores
 *            (optional) [K][n_th * n_lin * n_lin] every lattice candidate's raw score.  A raw
 *            score has the bits of the small-lattice search's with its default plan; two calls
 *            give the same bits.  Refused before anything is launched: a non-finite start
 *            (NDT2D_ERR_INVALID, the message says "start k"), no grid (NDT2D_ERR_NO_GRID), a
 *            lattice or beam count ndt2d_set_search / ndt2d_set_beams refuse (NDT2D_ERR_INVALID).
 *            n_starts == 0: NDT2D_OK, nothing done.
 *   set_timing / last_ms   HIP events around the search and the reduce launch of the last
 *            (chunk of a) match, off by default. */
typedef struct ndt2d_starts ndt2d_starts;
int ndt2d_starts_create(ndt2d_handle h, size_t max_starts, ndt2d_starts ** out);
int ndt2d_starts_destroy(ndt2d_starts * starts);
const char * ndt2d_starts_last_error(ndt2d_starts * starts);
int ndt2d_starts_match(ndt2d_starts * starts, const double * starts_xyt, size_t n_starts,
                       const double * beams_xy, size_t n_beams, const double * dth, size_t n_th,
                       const double * dlin, size_t n_lin, double * records_out,
                       double * all_scores);
int ndt2d_starts_set_timing(ndt2d_starts * starts, int enabled);
int ndt2d_starts_last_ms(ndt2d_starts * starts, float * search_ms, float * reduce_ms);

/* ---- wide search: the exhaustive lattice's winner by tile bounds (csrc/wide/) ----
 *
 * One scan, the grid INSTALLED in the context, one pose, a lattice too large to score whole (a
 * window of metres and radians for relocalisation or a loop closure after drift).  The record is
 * the one ndt2d_starts_match gives for this start on the same beams, dth and dlin -- best_score bit
 * for bit, the same best_index, the same near-tie mark -- but most candidates are never scored:
 *   image    pixel (i, j) of an image with origin grid origin - (W + P) and pitch P holds an upper
 *            bound on Cell::score(p) over the box [x_i - g, x_i + P + W + g] x [y_j - g, y_j + P + W + g],
 *            g = 1e-9 m: over the cells with n >= 5 the box touches, exp of the exact maximum of the
 *            cell's exponent over box and cell (each inflated by g), times 1 + 2^-40, plus 2^-1000
 *            (for values exp() leaves subnormal, where a relative inflation does nothing); 0
 *            where the box touches none.  A cell with a non-finite record is left out: a candidate that touches
 *            one scores NaN and cannot win.  FP64 in device memory.
 *   tiles    with tile_steps T the translation lattice of a theta step is cut into the index windows
 *            [ix0, min(ix0 + T, n_lin)) x [iy0, min(iy0 + T, n_lin)); a tile job is (theta step,
 *            tile), job = (ith * n_tiles + ix0 / T) * n_tiles + iy0 / T.  W is the widest
 *            dlin[last] - dlin[first] over the windows, P = max(W, cell_size / 4) / pixels_per_tile.
 *   bounds   a job's bound: every beam rotated as the searches rotate it, moved by (dlin[ix0],
 *            dlin[iy0]), looked up in the image (off the image, or NaN: 0), summed in FP64 in a
 *            fixed order.  It is never below the raw likelihood sum of a candidate of the tile.
 *   order    the jobs sorted by bound, descending; equal bounds in ascending job order.
 *   rounds   the sorted jobs are scored exactly in chunks (64, 128, ... up to max_tiles), a block
 *            per tile job; after each chunk one small read-back.  The call ends when the next
 *            bound is strictly below best_sum * (1 - 2^-35): every candidate within the near-tie
 *            tolerance (NDT2D_NEAR_TIE_REL) of the winner has been scored by then.  No winner yet
 *            (a map without cells): every tile is scored, the index is -1.
 * The covariance sums acc[10] need every candidate and are NOT made: a covariance for the winner
 * comes from ndt2d_refine (neighbourhood 9).  A near tie is marked, not settled.
 * An object of its own beside the context, as ndt2d_starts: it reads the grid installed at the
 * time of the call, installs nothing, launches on the context's current stream, and must be
 * destroyed before ndt2d_destroy(h).
 *
 *   create   max_tiles (1 .. 2^24): tile jobs of one exact launch at most.
 *   set_tile / tile   tile_steps 1 .. 32 (default NDT2D_WIDE_DEFAULT_TILE_STEPS), pixels_per_tile
 *            1 .. 8 (default NDT2D_WIDE_DEFAULT_PIXELS_PER_TILE); anything else: NDT2D_ERR_INVALID,
 *            the values stay.
 *   match    pose_xyt[3]; beams_xy: the subsampled robot-frame beams; dth[n_th] / dlin[n_lin] as
 *            for ndt2d_starts_match, dlin strictly ascending.  record_out[2] = {best_score,
 *            best_index (-1: none; + 0.5: near tie)} with the flat index of the FULL lattice
 *            (ith * n_lin^2 + ix * n_lin + iy); stats_out[2] (optional) = {tile jobs scored, tile
 *            jobs in all}; bounds_out[n_th * n_tiles^2] (optional) every job's bound;
 *            evaluated_out (optional) a byte per job, 1 = scored.  reuse_image = 1 is the caller's
 *            statement that the installed grid is that of this object's previous call: the image
 *            is kept when W and P are the same too.  Otherwise it is made inside the call: one more
 *            launch, no synchronisation.  Two calls give the same bits and score the same tiles.
 *            Refused before anything is launched (NDT2D_ERR_INVALID unless said otherwise), the
 *            message names the remedy: a non-finite pose; no grid (NDT2D_ERR_NO_GRID); a lattice or
 *            beam count ndt2d_set_search / ndt2d_set_beams refuse; dlin not strictly ascending; an
 *            image of more than 2^26 pixels; a box that spans more than 8 x 8 cells (the tile is then
 *            too coarse to prune anything); 2^31 tile jobs or more.
 *   read_image   info_out[8] = {nx, ny, origin_x, origin_y, P, W, g, 0} of the last image made and,
 *            data_out != NULL, its nx * ny values, row j after row j - 1 (capacity in doubles; too
 *            small: NDT2D_ERR_INVALID).  Before the first match: NDT2D_ERR_STATE.
 *   set_timing / last_ms   HIP events round the image, the bounds, the sort and the exact rounds
 *            (with their read-backs) of the last match, off by default. */
/* (measured: experiments/wide_search_timing.py; at linear resolutions coarser than 0.05 m fewer tile
 * steps keep a box within 8 x 8 cells of 0.25 m) */
#define NDT2D_WIDE_DEFAULT_TILE_STEPS 16
#define NDT2D_WIDE_DEFAULT_PIXELS_PER_TILE 4
typedef struct ndt2d_wide ndt2d_wide;
int ndt2d_wide_create(ndt2d_handle h, size_t max_tiles, ndt2d_wide ** out);
int ndt2d_wide_destroy(ndt2d_wide * wide);
const char * ndt2d_wide_last_error(ndt2d_wide * wide);
int ndt2d_wide_set_tile(ndt2d_wide * wide, uint32_t tile_steps, uint32_t pixels_per_tile);
int ndt2d_wide_tile(ndt2d_wide * wide, uint32_t * tile_steps, uint32_t * pixels_per_tile);
int ndt2d_wide_match(ndt2d_wide * wide, const double * pose_xyt, const double * beams_xy, size_t n_beams,
                     const double * dth, size_t n_th, const double * dlin, size_t n_lin, int reuse_image,
                     double * record_out, uint64_t * stats_out, double * bounds_out,
                     uint8_t * evaluated_out);
int ndt2d_wide_read_image(ndt2d_wide * wide, double * info_out, double * data_out, size_t capacity);
int ndt2d_wide_set_timing(ndt2d_wide * wide, int enabled);
int ndt2d_wide_last_ms(ndt2d_wide * wide, float * image_ms, float * bounds_ms, float * sort_ms,
                       float * exact_ms);

/* ---- batched scan tracking: K scans, each from its own pose (csrc/scans/) ----
 *
 * A job is a (scan, pose) pair; a call takes S scans and K jobs against the grid INSTALLED in the
 * context: what K calls of ndt2d_set_search_beams + ndt2d_match_launch(0, n_th) +
 * ndt2d_match_fetch give, each with its job's beams and pose, in one upload, the search launches
 * over (theta step x job), one reduction and one read-back.  The reference's localisation branch
 * (src/ndt_mapper.cpp:547-566) for many scans at once: a fleet of robots on one shared map, a
 * recorded bag replayed against a loaded map, every scan of a graph matched again after an
 * optimisation.  ndt2d_starts_match is the case S = 1.
 * An object of its own beside the context, as ndt2d_starts: it reads the grid installed at the
 * time of the call (any install path, any size or origin), installs nothing, launches on the
 * context's current stream, and must be destroyed before ndt2d_destroy(h).
 *
 *   create   max_jobs (1 .. 4,096): jobs of one chunk; a call with more is processed in chunks
 *            inside the call.  Chunking changes no bit.
 *   match    jobs_xyt[K][3]; job_scan[K]: the scan of job k (several jobs may name one scan: its
 *            beams travel once; a scan no job names is legal and is not uploaded), NULL: job k
 *            uses scan k and n_scans must equal n_jobs.  beams_xy: the already subsampled
 *            robot-frame beams of all scans, scan s = beams_xy[2 * beam_offsets[s] ..
 *            2 * beam_offsets[s + 1]), beam_offsets[n_scans + 1] non-decreasing; beams are taken
 *            as given ("Points off the grid" below).  dth[n_th] / dlin[n_lin]: the visited
 *            offsets (ndt2d_set_search).  cos / sin of theta_k + dth[i] come from the host libm
 *            inside the call.  records_out and all_scores (optional) have the layouts of
 *            ndt2d_starts_match, by job in the caller's order.  The partial sums of a raw score
 *            follow from the beam count of the job's scan, so a raw score has the bits of the
 *            small-lattice search's with its default plan; the jobs of a chunk are searched with
 *            one launch per number of partial sums present (one when every scan has the same
 *            count, eight at most).  A job's bits do not depend on the other jobs.
 *            Refused with NDT2D_ERR_INVALID before anything is launched: a non-finite job pose or
 *            job_scan[k] >= n_scans (the message says "job k"), a scan with 0 or more than 2^20
 *            beams or beam_offsets that decrease ("scan s"), a lattice ndt2d_set_search refuses,
 *            job_scan == NULL with n_scans != n_jobs.  No grid: NDT2D_ERR_NO_GRID.
 *            n_jobs == 0: NDT2D_OK, nothing done.
 *   set_timing / last_ms   HIP events around the search launches and the reduce launch of the
 *            last (chunk of a) match, off by default. */
typedef struct ndt2d_scans ndt2d_scans;
int ndt2d_scans_create(ndt2d_handle h, size_t max_jobs, ndt2d_scans ** out);
int ndt2d_scans_destroy(ndt2d_scans * scans);
const char * ndt2d_scans_last_error(ndt2d_scans * scans);
int ndt2d_scans_match(ndt2d_scans * scans, const double * jobs_xyt, const uint32_t * job_scan,
                      size_t n_jobs, const double * beams_xy, const size_t * beam_offsets,
                      size_t n_scans, const double * dth, size_t n_th, const double * dlin,
                      size_t n_lin, double * records_out, double * all_scores);
int ndt2d_scans_set_timing(ndt2d_scans * scans, int enabled);
int ndt2d_scans_last_ms(ndt2d_scans * scans, float * search_ms, float * reduce_ms);

/* ---- Newton NDT registration: K (scan, pose) jobs refined in one launch (csrc/refine/) ----
 *
 * Every search above ends on the lattice: its pose is quantised to the lattice's pitch.  A job
 * here is a (scan, pose) pair as in ndt2d_scans_match; for each, a damped Newton iteration on the
 * scan's NDT score against the grid INSTALLED in the context runs from the job's pose to the
 * optimum under it.  One call is one upload, ONE kernel launch for the whole iteration of all
 * jobs of a chunk (a workgroup per job loops until its job stops) and one read-back.
 * An object of its own beside the context, as ndt2d_scans: it reads the grid installed at the
 * time of the call (any install path, any size or origin), installs nothing, launches on the
 * context's current stream, and must be destroyed before ndt2d_destroy(h).
 *
 * The objective.  For a pose p = (x, y, theta) and the job's beams b_i (robot frame, already
 * subsampled), with c = cos theta, s = sin theta:
 *     q_i = (c bx - s by + x,  s bx + c by + y)
 *     the cell of q_i is NDT::getIndex's; the beam counts only if the cell can score (n >= 5)
 *     d = q - mean,  u = I d,  e = exp(-1/2 d^T I d)      I: the cell's information matrix
 *         (the records hold h = -1/2 I: the exponent is Cell::score's, I = -2 h exactly, and
 *          u_0 = I00 d0 + I01 d1, u_1 = I01 d0 + I11 d1)
 *     r = dq/dtheta   = (-s bx - c by,  c bx - s by)
 *     w = d2q/dtheta2 = (-c bx + s by, -s bx - c by)
 *     a = (u_0, u_1, u_0 r_0 + u_1 r_1)
 *     M = [[I00, I01, (I r)_0], [., I11, (I r)_1], [., ., (r_0 (I r)_0 + r_1 (I r)_1) + (u_0 w_0 + u_1 w_1)]]
 *     f    = -sum e                    (f / N is what ScanMatcherNDT::scorePoints returns)
 *     g_j  =  sum e a_j
 *     H_jk =  sum e (-(a_j a_k) + M_jk)          six entries: xx, xy, xt, yy, yt, tt
 * Ten sums; a beam's ten terms are added by thread (beam mod 256) in beam order, the 256 partial
 * sums of each by a fixed tree, so two calls give the same bits.  The cell borders are
 * discontinuities of f (the reference's NDT has no overlapping or interpolated cells); the
 * iteration only ever accepts a pose that lowers f.
 *
 * The neighbourhood (ndt2d_refine_set_neighbourhood: 1, the default and the objective above, or 9).
 * With 9 a point is scored against the 3 x 3 cells round it (what NDT implementations call direct
 * neighbours), which takes the jumps at the cell borders down by two to three orders of magnitude:
 *     a point's own cell (gx, gy) is NDT::getIndex's; a point off the grid (NaN or infinite
 *         included) contributes nothing
 *     neighbour j = 0 .. 8 is (dy, dx) = (j / 3 - 1, j % 3 - 1) from the own cell; j = 4 is the own cell
 *     a neighbour counts only if 0 <= gx + dx < size_x, 0 <= gy + dy < size_y -- clipped on
 *         (gx, gy), never on the flat index -- and its cell can score (n >= 5)
 *     each counting neighbour adds the ten terms above, with d = q - that cell's mean and I that
 *         cell's information matrix; no weighting, no normalisation
 * A job's items are (beam, neighbour) pairs, i = K beam + j for a neighbourhood of K cells; item
 * i's ten terms are added by thread (i mod 256) in ascending i, the 256 partial sums by the same
 * fixed tree.  For K = 1 this is the order above, and the bits are the same.  f == 0 over all
 * items: NO_OVERLAP; f not finite -- a degenerate neighbour as well as a degenerate own cell --:
 * NOT_FINITE.  The iteration is the same.  f / N is then no longer what scorePoints returns.
 *
 * The iteration.
 *   1. Evaluate (f, g, H) at the start: evals = 1.  f == 0 (no beam scores): NO_OVERLAP; f not
 *      finite: NOT_FINITE; either way the pose is returned bit for bit.
 *   2. lambda = 0.
 *   3. While evals < max_evals:
 *        D_j = max(|H_jj|, 1e-12); solve (H + lambda diag D) delta = -g by 3 x 3 Cholesky; on a
 *        pivot that is not > 0: lambda = max(10 lambda, 1e-3) and again, past 1e12: STALLED.
 *        |dx| < tol_lin and |dy| < tol_lin and |dtheta| < tol_ang: CONVERGED.
 *        Evaluate at p + delta (theta is not normalised): evals += 1.
 *        f' < f: accept p, f, g, H; lambda = lambda / 10, and 0 once that is <= 1e-9.
 *        else:   lambda = max(10 lambda, 1e-3), past 1e12: STALLED.
 *   4. Leaving the loop by count: MAX_EVALS (max_evals == 1 is the evaluation alone).
 * The returned (f, g, H) are those of the returned pose; f never increases.  cos / sin of the
 * START heading come from the host libm inside the call, those of later headings from the
 * device's sincos.
 *
 *   create   max_jobs (1 .. 4,096): jobs of one chunk; a call with more is processed in chunks
 *            inside the call.  Chunking changes no bit; a job's bits do not depend on the other
 *            jobs.
 *   run      jobs_xyt, job_scan, beams_xy, beam_offsets, n_scans: ndt2d_scans_match's conventions
 *            (shared scans travel once, a scan no job names is legal and is not uploaded,
 *            job_scan == NULL: job k uses scan k and n_scans must equal n_jobs; beams are taken
 *            as given, "Points off the grid" below).  max_evals >= 1; tol_lin (m) and tol_ang
 *            (rad) >= 0 (the matcher layer's defaults: 32, 1e-6, 1e-6).
 *            records_out[K][NDT2D_REFINE_RECORD_DOUBLES], by job in the caller's order:
 *            {x, y, theta | f_start, f | g[3] | H xx, xy, xt, yy, yt, tt | evals, accepted
 *            steps, status (NDT2D_REFINE_*), the last lambda}.
 *            Refused with NDT2D_ERR_INVALID before anything is launched: a non-finite job pose or
 *            job_scan[k] >= n_scans (the message says "job k"), a scan with 0 or more than 2^20
 *            beams or beam_offsets that decrease ("scan s"), max_evals == 0, a tolerance that is
 *            negative or not finite, job_scan == NULL with n_scans != n_jobs.  No grid:
 *            NDT2D_ERR_NO_GRID.  n_jobs == 0: NDT2D_OK, nothing done.
 *   set_timing / last_ms   HIP events around the kernel launch and the read-back of the last
 *            (chunk of a) run, off by default.
 *   set_neighbourhood / neighbourhood   cells: 1 (the default) or 9, for the later runs of this
 *            object; anything else is NDT2D_ERR_INVALID with a message, and the value stays.
 *   covariance   host arithmetic only: no object, no device, usable without a GPU.  H6: a
 *            record's six entries xx, xy, xt, yy, yt, tt; cov9_out: H^-1, row-major 3 x 3, symmetric
 *            bit for bit, by the 3 x 3 Cholesky of the iteration with lambda = 0 and no scaling.
 *            NDT2D_ERR_STATE, cov9_out untouched: an entry of H (or of the inverse) is not finite,
 *            or a pivot is not > 0 (H is not positive definite: the pose is no minimum of f, or a
 *            direction is not observed).  NDT2D_ERR_INVALID: a NULL argument.
 *            Why H^-1 is a covariance: near the optimum e = exp(-1/2 d^T I d) ~ 1 - 1/2 d^T I d, so
 *            f ~ -N + 1/2 sum d^T I d and H -> sum J^T I J, J = dq / d(x, y, theta): the information
 *            matrix of the point-to-distribution residuals under the map's own Gaussians.  H is
 *            the Hessian of the SUM (the record's), not of f / N: from the matcher layer's H / N,
 *            multiply by N first.  With neighbourhood 1 the returned H describes f only inside
 *            the current cell pattern; a covariance is meant to be taken from neighbourhood 9. */
#define NDT2D_REFINE_RECORD_DOUBLES 18
#define NDT2D_REFINE_CONVERGED 0    /* the Newton step fell below the tolerances */
#define NDT2D_REFINE_MAX_EVALS 1    /* max_evals evaluations were made */
#define NDT2D_REFINE_STALLED 2      /* lambda passed 1e12: no step lowers f */
#define NDT2D_REFINE_NO_OVERLAP 3   /* no beam of the scan scores at the start pose */
#define NDT2D_REFINE_NOT_FINITE 4   /* f at the start pose is not finite (a degenerate cell) */
typedef struct ndt2d_refine ndt2d_refine;
int ndt2d_refine_create(ndt2d_handle h, size_t max_jobs, ndt2d_refine ** out);
int ndt2d_refine_destroy(ndt2d_refine * refine);
const char * ndt2d_refine_last_error(ndt2d_refine * refine);
int ndt2d_refine_run(ndt2d_refine * refine, const double * jobs_xyt, const uint32_t * job_scan,
                     size_t n_jobs, const double * beams_xy, const size_t * beam_offsets,
                     size_t n_scans, uint32_t max_evals, double tol_lin, double tol_ang,
                     double * records_out);
int ndt2d_refine_set_timing(ndt2d_refine * refine, int enabled);
int ndt2d_refine_last_ms(ndt2d_refine * refine, float * kernel_ms, float * fetch_ms);
int ndt2d_refine_set_neighbourhood(ndt2d_refine * refine, uint32_t cells);
int ndt2d_refine_neighbourhood(ndt2d_refine * refine, uint32_t * out);
int ndt2d_refine_covariance(const double * H6, double * cov9_out);

/* ---- Newton NDT registration on each loop-closure candidate's own map (csrc/closure/) ----
 *
 * The loop-closure constraint (makeConstraint, src/ndt_mapper.cpp:658) is matched against a
 * candidate's own map of one or two old scans, which ndt2d_closure_match builds in the closure's
 * buffers and drops.  ndt2d_closure_refine runs the registration above on such maps: per chunk
 * one upload, the build launch of ndt2d_closure_match for the candidates the jobs name (a
 * candidate no job names is not built), ONE launch of the refinement -- a workgroup per job, on
 * the packed records and the cell -> record table of its candidate's slot -- and one read-back.
 * The kernel is the one of ndt2d_refine_run (csrc/refine/ndt2d_refine.hip), instantiated on the
 * slots; nothing of the grid installed in the context is read or changed.
 *
 *   candidates   cand_offsets, ids, poses_xyt, ndt_resolution, range_max as ndt2d_closure_match
 *                takes them, with everything it refuses about a candidate.
 *   scans, jobs  beams_xy, beam_offsets, n_scans, jobs_xyt, job_scan, max_evals, tol_lin, tol_ang
 *                as ndt2d_refine_run takes them, with everything it refuses; job_candidate[k]: the
 *                candidate job k is refined on (NULL: job k uses candidate k, n_jobs must equal
 *                n_candidates).  A job_scan or job_candidate out of range: NDT2D_ERR_INVALID, the
 *                message names the job, nothing is launched.
 *   records_out  [n_jobs][NDT2D_REFINE_RECORD_DOUBLES] in ndt2d_refine_run's layout, in job order.
 *   bits         a job's record has the bits ndt2d_refine_run gives for the same scan and pose on
 *                the grid ndt2d_scanstore_build installs for the candidate, neighbourhood for
 *                neighbourhood; it depends on its scan, its pose and its candidate's scans and
 *                poses alone, not on the other jobs or the chunks.
 *   chunks       candidates in ascending index among those named, at most max_candidates
 *                (ndt2d_closure_create) candidates and 4,096 jobs a launch; a candidate with more
 *                jobs continues in launches of its own (csrc/closure/ndt2d_closure_jobs.h).
 *   set_neighbourhood / neighbourhood   1 (the default) or 9 cells per point, the rule of
 *                ndt2d_refine_set_neighbourhood.
 *   ndt2d_closure_last_ms   reports the last call of either kind: the build, and the launch
 *                behind it (the search of a match, the refinement of a refine). */
int ndt2d_closure_refine(ndt2d_closure * closure, size_t n_candidates, const size_t * cand_offsets,
                         const size_t * ids, const double * poses_xyt, double ndt_resolution,
                         double range_max, const double * jobs_xyt, const uint32_t * job_scan,
                         const uint32_t * job_candidate, size_t n_jobs, const double * beams_xy,
                         const size_t * beam_offsets, size_t n_scans, uint32_t max_evals,
                         double tol_lin, double tol_ang, double * records_out);
int ndt2d_closure_set_neighbourhood(ndt2d_closure * closure, uint32_t cells);
int ndt2d_closure_neighbourhood(ndt2d_closure * closure, uint32_t * out);

/* ---- Match verification: inlier, unseen and pierced beams of K (scan, pose) jobs in one launch
 *      (csrc/verify/) ----
 *
 * Every search and the registration above turn a scan and a guess into a pose and one number, the
 * mean NDT score.  This says which beams of the scan the map explains at that pose: one verdict per
 * beam, integer counts per job.  A job is a (scan, pose) pair in ndt2d_refine_run's conventions.
 * One call is one upload, ONE kernel launch per chunk (a workgroup per job) and one read-back.  An
 * object of its own beside the context, as ndt2d_refine: it reads the grid installed at the time
 * of the call, installs nothing, launches on the context's current stream, and must be destroyed
 * before ndt2d_destroy(h).  A job's result depends on its scan, its pose, the grid and the
 * parameters alone: not on the other jobs or the chunking.  No policy: nothing is accepted or
 * rejected here.
 *
 * Job and beam.  For the job's pose (x, y, theta), c = cos theta and s = sin theta come from the
 * host libm inside the call.  A beam b (robot frame, taken as given) becomes
 *     q = (c bx - s by + x,  s bx + c by + y)
 * as the registration forms it.  The beam's own cell is NDT::getIndex's of q.
 *
 * Class of a beam (the two low bits of its byte):
 *     0  NDT2D_BEAM_OFF      q is off the grid (NaN and infinite points included)
 *     1  NDT2D_BEAM_UNSEEN   q is on the grid, and no cell of the neighbourhood can score (n >= 5)
 *     3  NDT2D_BEAM_INLIER   m2 <= gate_inlier
 *     2  NDT2D_BEAM_OUTLIER  otherwise: !(m2 <= gate_inlier); a NaN m2 (a degenerate cell) is an outlier
 * The neighbourhood is 1 cell (the beam's own) or 9 (the 3 x 3 round it), by the rule of
 * ndt2d_refine_set_neighbourhood: neighbour j = 0 .. 8 is (dy, dx) = (j / 3 - 1, j % 3 - 1) from the
 * own cell (gx, gy), and counts only if 0 <= gx + dx < size_x, 0 <= gy + dy < size_y -- clipped on
 * (gx, gy), never on the flat index -- and its cell can score.  For a counting cell with mean m and
 * information I, d = q - m and
 *     m2 = d^T I d = -2 x (Cell::score's exponent on the record's h = -1/2 I;  I = -2 h exactly)
 * A beam's m2 is the minimum over its counting neighbours in ascending j: a neighbour replaces the
 * one held when its m2 is below the held one, or is NaN while the held one is not (a NaN stays:
 * numpy's argmin).  Ties go to the lowest j.
 *
 * The ray.  It is walked only when rays are enabled, the beam is not OFF and the job's origin cell
 * -- NDT::getIndex of (x, y) -- is on the grid.  Its cells are those of the integer line from the
 * origin cell (ox, oy) to the beam's own cell (gx, gy) in the all-octant error form the occupancy
 * grid uses (src/occupancy_grid.cpp:93-131):
 *     dx = |gx - ox|, dy = -|gy - oy|, sx, sy = the signs, err = dx + dy; the cell (ox, oy) is visited;
 *     at a visited cell: it is the end cell: stop.
 *         2 err >= dy: x is the end's: stop;  else err += dy, x += sx
 *         2 err <= dx (the err just updated): y is the end's: stop;  else err += dx, y += sy
 *     the cell now reached is visited.  At most dx - dy + 1 cells are visited.  (As there, a walk
 *     can stop one step short of the end cell; that is inside the end's own 3 x 3, see below.)
 * A visited cell is TESTED when it is not the origin cell, its Chebyshev distance to the end cell
 * is > 1 (the end's own 3 x 3 belongs to the end point, not to the ray) and it can score.  For a
 * tested cell with mean m and information I, o = (x, y), in this operation order:
 *     u = q - o;  w = m - o
 *     Iu = (I00 ux + I01 uy,  I01 ux + I11 uy)
 *     D = ux Iu_0 + uy Iu_1                       (u^T I u)
 *     N = wx Iu_0 + wy Iu_1                       (u^T I w)
 *     t = N / D;  t = 0 when !(D > 0);  then !(t >= 0) -> 0 (a NaN too), t > 1 -> 1
 *     r = w - t u;  Ir as Iu;  r^T I r = rx Ir_0 + ry Ir_1
 *     the cell PIERCES when r^T I r <= gate_pierce
 * -- the segment from the robot to the beam's end passes through the cell's Gaussian.  The walk
 * stops at the first piercing cell: bit 2 (NDT2D_BEAM_PIERCED = 4) of the beam's byte is set and
 * the cell's flat index recorded.  (A grid side above 2^24 cells with rays enabled is refused.)
 *
 *   create   max_jobs (1 .. 4,096): jobs of one chunk; more are processed in chunks inside the
 *            call (a chunk also ends where its jobs' beams pass 2^24).  Chunking changes no output.
 *   run      jobs_xyt, job_scan, beams_xy, beam_offsets, n_scans: ndt2d_refine_run's conventions
 *            (shared scans travel once, a scan no job names is legal and is not uploaded,
 *            job_scan == NULL: job k uses scan k and n_scans must equal n_jobs).
 *            records_out[K][NDT2D_VERIFY_RECORD_U32], by job in the caller's order:
 *            {n_beams, n_off, n_unseen, n_outlier, n_inlier, n_pierced, n_walked, 0}; n_walked:
 *            the beams whose ray was walked.  Integers: no summation order matters.
 *            Optional, each may be NULL, per beam, job after job in the caller's order -- job k's
 *            beams start at the sum of the earlier jobs' scan lengths:
 *              beam_class_out   uint8: class | NDT2D_BEAM_PIERCED
 *              beam_m2_out      double: the beam's m2; OFF and UNSEEN give +inf
 *              beam_cells_out   uint32[.][2]: the cell whose m2 won | the first piercing cell;
 *                               NDT2D_VERIFY_NO_CELL: none
 *            Refused with NDT2D_ERR_INVALID before anything is launched: everything
 *            ndt2d_refine_run refuses about jobs and scans, with "job k" or "scan s" in the
 *            message.  No grid: NDT2D_ERR_NO_GRID.  n_jobs == 0: NDT2D_OK, nothing done.
 *   set_neighbourhood / neighbourhood   1 (the default at this layer) or 9
 *   set_gates / gates   gate_inlier (default 9.0) and gate_pierce (default 1.0): each >= 0 and finite
 *   set_rays / rays     the ray walk on (the default) or off: enabled is 0 or 1
 *            Anything else: NDT2D_ERR_INVALID with a message, and the old values stay.  The
 *            defaults are starting values, not tuned.
 *   set_timing / last_ms   HIP events around the kernel launch and the read-back of the last
 *            (chunk of a) run, off by default. */
#define NDT2D_VERIFY_RECORD_U32 8
#define NDT2D_BEAM_OFF 0
#define NDT2D_BEAM_UNSEEN 1
#define NDT2D_BEAM_OUTLIER 2
#define NDT2D_BEAM_INLIER 3
#define NDT2D_BEAM_PIERCED 4        /* bit 2 of a beam's byte: its ray met a piercing cell */
#define NDT2D_VERIFY_NO_CELL 0xFFFFFFFFu
typedef struct ndt2d_verify ndt2d_verify;
int ndt2d_verify_create(ndt2d_handle h, size_t max_jobs, ndt2d_verify ** out);
int ndt2d_verify_destroy(ndt2d_verify * verify);
const char * ndt2d_verify_last_error(ndt2d_verify * verify);
int ndt2d_verify_run(ndt2d_verify * verify, const double * jobs_xyt, const uint32_t * job_scan,
                     size_t n_jobs, const double * beams_xy, const size_t * beam_offsets,
                     size_t n_scans, uint32_t * records_out, uint8_t * beam_class_out,
                     double * beam_m2_out, uint32_t * beam_cells_out);
int ndt2d_verify_set_neighbourhood(ndt2d_verify * verify, uint32_t cells);
int ndt2d_verify_neighbourhood(ndt2d_verify * verify, uint32_t * out);
int ndt2d_verify_set_gates(ndt2d_verify * verify, double gate_inlier, double gate_pierce);
int ndt2d_verify_gates(ndt2d_verify * verify, double * gate_inlier_out, double * gate_pierce_out);
int ndt2d_verify_set_rays(ndt2d_verify * verify, int enabled);
int ndt2d_verify_rays(ndt2d_verify * verify, int * out);
int ndt2d_verify_set_timing(ndt2d_verify * verify, int enabled);
int ndt2d_verify_last_ms(ndt2d_verify * verify, float * kernel_ms, float * fetch_ms);

/* ---- Match verification on each loop-closure candidate's own map (csrc/closure/) ----
 *
 * A loop-closure match is made against the candidate's own map of one or two old scans, which
 * ndt2d_closure_match and ndt2d_closure_refine build in the closure's buffers and drop.
 * ndt2d_closure_verify runs the verification above on such maps: per chunk one upload, the build
 * launch of ndt2d_closure_match for the candidates the jobs name (a candidate no job names is not
 * built), ONE launch of the verification -- a workgroup per job, on the packed records and the
 * cell -> record table of its candidate's slot -- and one read-back.  The kernel is the one of
 * ndt2d_verify_run (csrc/verify/ndt2d_verify.hip), instantiated on the slots; nothing of the grid
 * installed in the context is read or changed, and no installed grid is no error here.  A verdict,
 * not a policy: nothing is accepted or rejected.
 *
 *   candidates   cand_offsets, ids, poses_xyt, ndt_resolution, range_max as ndt2d_closure_match
 *                takes them, with everything it refuses about a candidate.
 *   scans, jobs  beams_xy, beam_offsets, n_scans, jobs_xyt, job_scan as ndt2d_verify_run takes
 *                them, with everything it refuses; job_candidate[k]: the candidate job k is
 *                verified on (NULL: job k uses candidate k, n_jobs must equal n_candidates).  A
 *                job_scan or job_candidate out of range: NDT2D_ERR_INVALID, the message names the
 *                job ("job k").  A slot grid side above 2^24 cells with rays enabled:
 *                NDT2D_ERR_INVALID.  A refused call launches nothing and leaves the outputs as they
 *                were.
 *   outputs      records_out, beam_class_out, beam_m2_out, beam_cells_out in ndt2d_verify_run's
 *                layouts and job order; the per-beam arrays are optional, each may be NULL.
 *   bits         a job's record and per-beam outputs are what ndt2d_verify_run gives for the same
 *                scan, pose and parameters on the grid ndt2d_scanstore_build installs for that
 *                candidate; a job depends on nothing but its scan, its pose, its candidate and
 *                the parameters: not on the other jobs or the chunks.
 *   chunks       the plan of ndt2d_closure_refine (csrc/closure/ndt2d_closure_jobs.h): at most
 *                max_candidates candidates and 4,096 jobs a launch; a chunk also closes where its
 *                jobs' per-beam results pass 2^24 (a job more is taken whole).
 *   set_verify_neighbourhood / _gates / _rays and their getters   the parameters of this call,
 *                kept on the closure object with ndt2d_verify's rules, defaults (1 cell, 9.0 and
 *                1.0, rays on) and refusals; the neighbourhood is apart from the refinement's
 *                ndt2d_closure_set_neighbourhood.
 *   ndt2d_closure_last_ms   after this call: the build and the verify launch of its last chunk. */
int ndt2d_closure_verify(ndt2d_closure * closure, size_t n_candidates, const size_t * cand_offsets,
                         const size_t * ids, const double * poses_xyt, double ndt_resolution,
                         double range_max, const double * jobs_xyt, const uint32_t * job_scan,
                         const uint32_t * job_candidate, size_t n_jobs, const double * beams_xy,
                         const size_t * beam_offsets, size_t n_scans, uint32_t * records_out,
                         uint8_t * beam_class_out, double * beam_m2_out, uint32_t * beam_cells_out);
int ndt2d_closure_set_verify_neighbourhood(ndt2d_closure * closure, uint32_t cells);
int ndt2d_closure_verify_neighbourhood(ndt2d_closure * closure, uint32_t * out);
int ndt2d_closure_set_verify_gates(ndt2d_closure * closure, double gate_inlier, double gate_pierce);
int ndt2d_closure_verify_gates(ndt2d_closure * closure, double * gate_inlier_out,
                               double * gate_pierce_out);
int ndt2d_closure_set_verify_rays(ndt2d_closure * closure, int enabled);
int ndt2d_closure_verify_rays(ndt2d_closure * closure, int * out);

/* ---- Pose graph: optimise scan poses against the constraints, K masks in one launch
 *      (csrc/posegraph/) ----
 *
 * What the loop-closure thread does with its constraints (src/ndt_mapper.cpp:680,
 * src/ceres_solver.cpp:50-120): move the scan poses so that the relative poses the constraints
 * measured are met as well as their weights allow.  An object of its own beside the context, as
 * ndt2d_refine: it launches on the context's current stream and must be destroyed before
 * ndt2d_destroy(h).  K jobs share one graph; a job is a mask over the constraints (the question
 * "is this closure consistent with the others?" is the solve with and without it).  One call is ONE
 * launch of the solver per chunk, a workgroup per job; nothing is asked of the host between the
 * iterations.  Ceres is not reproduced step by step: the contract is the minimiser and the rules below.
 *
 * The problem.  n poses (x, y, theta) and m constraints {begin, end, transform[3], information[9]
 * row-major}; begin and end index the poses, as scans[constraint->begin] does.  Pose `fixed` is
 * held (the reference holds scans[0]).
 *
 * The residual of a constraint a = begin, b = end with transform t
 * (include/ndt_2d/ceres_solver_pose.hpp:86-108), R(.) the rotation:
 *     e_xy    = R(theta_a)^T (p_b - p_a) - t_xy
 *     e_theta = Normalize((theta_b - theta_a) - t_theta)
 *     Normalize(v) = v - 2pi floor((v + pi) / 2pi), 2pi formed as 2.0 * pi: into [-pi, pi)
 *     r = W e
 * Normalize uses IEEE + - x / and floor only and the unit is compiled without contraction: the
 * unweighted e_theta has the bits a float64 restatement gives.  cos and sin of theta_a are the
 * device library's.
 *
 * The weighting.  L: the lower Cholesky factor of `information`, computed on the host at upload.
 *     "reference"    (default) W = L, what src/ceres_solver.cpp:132 passes as the "square root
 *                    information".  A quirk: the cost is then e^T L^T L e, which is NOT
 *                    e^T information e (= e^T L L^T e) unless L is diagonal.
 *     "information"  W = L^T: the cost is e^T information e.
 * A constraint whose information gives a Cholesky pivot <= 0 or not finite (not symmetric positive
 * definite as far as the factorisation can tell; Eigen's llt() goes on silently there, and the
 * zeros of a default-constructed Constraint are such a case) is refused.  Only the lower triangle
 * is read.
 *
 * The cost of a job: F = 1/2 sum |r_c|^2 over its enabled constraints; chi2_c = |r_c|^2.
 *
 * The Jacobians are analytic (csrc/posegraph/ndt2d_posegraph_fn.h), with c = cos theta_a,
 * s = sin theta_a and (ex, ey) = R(theta_a)^T (p_b - p_a):
 *     A = de/d(pose a) = [-c -s ey; s -c -ex; 0 0 -1]     B = de/d(pose b) = [c s 0; -s c 0; 0 0 1]
 *
 * The solver.  Levenberg-Marquardt: each iteration solves (H + lambda D) delta = -g, H = J^T J,
 * g = J^T r, D = diag(H) clamped to [1e-6, 1e32], by conjugate gradients that never form H, with
 * the 3 x 3 diagonal blocks of H + lambda D as preconditioner.  The trial point x + delta is
 * accepted when the gain ratio (F(x) - F(x + delta)) / (model decrease) is above 1e-3 -- or when
 * |F(x) - F(x + delta)| is below 256 eps F, where the ratio is the rounding of the cost's own sum
 * and the (positive) model decrease decides.  The damping update, the CG forcing term and the CG
 * cap are the implementation's (the kernel's head says which).  What follows from the cap,
 * min(3 n + 16, 8192) CG iterations per LM iteration: on a small ill-conditioned graph (24 poses with
 * kappa(H) ~ 1e7: anisotropic information) a "jacobi" solve needs more, the steps are then truncated
 * CG steps, and the LM iterations are many -- 129 where the direct solve takes 11, and 266 under Huber,
 * beyond Ceres's default max_iterations of 100, where the status is then
 * NDT2D_POSEGRAPH_MAX_ITERATIONS.  "chain", the direct and the sparse solve do not have it.
 * Stop rules, each evaluated in the kernel, a tolerance of 0 disables its rule:
 *     max_iterations          iterations made, accepted or not      NDT2D_POSEGRAPH_MAX_ITERATIONS
 *     gradient_tolerance      |g|_inf <= it, at the start or after an accepted step
 *                                                                    NDT2D_POSEGRAPH_CONVERGED_GRADIENT
 *     function_tolerance      |F_before - F| <= it x F_before after an accepted step
 *                                                                    NDT2D_POSEGRAPH_CONVERGED_COST
 *     parameter_tolerance     |delta|_2 <= it x (|x|_2 + it)         NDT2D_POSEGRAPH_CONVERGED_STEP
 *     a start cost that is not finite: NDT2D_POSEGRAPH_FAILED, the job's start poses are returned.
 * Ceres's defaults are 100 (src/ceres_solver.cpp:39), 1e-10, 1e-6, 1e-8.
 *
 * What a result depends on: the graph, the job's mask and the parameters -- not the other jobs, the
 * chunking or the run: bit-identical run to run.  No floating-point atomics: a node's sums are
 * gathers over its incident constraints in ascending constraint index, dot products are reduced in
 * a fixed tree.  A node with no enabled constraint in a job, and the fixed node, keep their poses
 * bit for bit.  A component not connected to the fixed pose has no unique minimiser; the damped
 * system is still definite, and a minimiser is returned.
 *
 *   create     max_nodes (1 .. 2^30), max_constraints (0 .. 2^30), max_jobs (1 .. 65,535: jobs of
 *              one chunk; more are processed in chunks inside the call, which changes no output).
 *   set_graph  Refused with NDT2D_ERR_INVALID before anything changes, the message names the
 *              index: n == 0 (the reference returns false for no scans), sizes beyond the
 *              capacities, fixed >= n, a non-finite pose ("pose i"), and per constraint
 *              ("constraint c") an index out of range, begin == end, a non-finite transform or
 *              information, an information that is not positive definite.  A refused graph leaves
 *              the one in place.  m == 0 or n == 1 is legal: nothing moves, CONVERGED_GRADIENT.
 *   set_weighting / weighting   "reference" or "information"; anything else: NDT2D_ERR_INVALID.
 *   ndt2d_pose_graph_set_preconditioner / ndt2d_pose_graph_preconditioner   (so named, not
 *              ndt2d_posegraph_*: the entry points of that prefix are a closed list of ten, which
 *              tests/test_posegraph_host.py holds the unit and the bindings to; these two act on
 *              the same object)  the CG's preconditioner M, z = M^-1 r: "jacobi" (the
 *              default: the 3 x 3 diagonal blocks above) or "chain"; anything else:
 *              NDT2D_ERR_INVALID.  Kept across set_graph.  "chain": with a job's free nodes the
 *              active ones (not the fixed one, and with at least one enabled constraint), M is the
 *              block-tridiagonal band of H + lambda D over the nodes in node order.  Its diagonal
 *              blocks are the job's full 3 x 3 blocks of H plus lambda x clamp(diag), as "jacobi"
 *              has them.  Its block (i, i + 1) is the sum, in ascending constraint index, over the
 *              enabled constraints that join nodes i and i + 1 (begin = i, end = i + 1 or the
 *              reverse, duplicates too) of (W E_i)^T (W E_{i+1}), E_i the constraint's Jacobian by
 *              node i; it is zero when either node is not free: the chain breaks there.  A node
 *              that is not free has z = 0.  M is J_c^T J_c of the neighbour constraints plus a
 *              positive semidefinite block diagonal plus lambda D > 0: symmetric positive definite
 *              for every mask.  z = M^-1 r exactly, by block cyclic reduction of 3 x 3 blocks
 *              (csrc/posegraph/ndt2d_posegraph_chain.h) for any n: M is factored once per
 *              iteration, the factors are applied once per CG iteration, ceil(log2 n) levels down
 *              and up.  Should a pivot block not be finite and positive definite, that iteration
 *              uses the "jacobi" blocks.  Graphs whose odometry runs along the node order (the
 *              mapper's: begin = i, end = i + 1) are what it is for: what M leaves out of
 *              H + lambda D has rank <= 6 per enabled constraint between nodes that are not
 *              neighbours.  The stop rules, the record, cg_iterations and the determinism above
 *              are the same; the minimiser reached is the same within the tolerances, not the bits.
 *              The workspace on the device is 83 doubles a node and job instead of 41.
 *   evaluate  enabled[K][m] bytes (non-zero: on) or NULL for every constraint on; at the graph's
 *              poses: cost_out[K]; optional chi2_out[K][m] and residuals_out[K][m][6] = e then r,
 *              of every constraint, enabled or not (the mask selects what F sums).
 *   solve      poses_out[K][n][3]; records_out[K][NDT2D_POSEGRAPH_RECORD_DOUBLES] = {status,
 *              iterations, cg_iterations, initial_cost, final_cost, final |g|_inf}; optional
 *              chi2_out[K][2][m]: every constraint's chi2 at the start and at the job's final poses
 *              (a switched-off closure's chi2 against the others' solution is the verdict on it;
 *              no policy is applied).  initial_cost is evaluate's F bit for bit.
 *              n_jobs == 0: NDT2D_OK, nothing done.  Before set_graph: NDT2D_ERR_STATE.  A negative
 *              or non-finite tolerance: NDT2D_ERR_INVALID.
 *   set_timing / last_ms   HIP events around the kernel launches and the read-back of the last
 *              (chunk of a) call, off by default.
 *
 * Robust losses (ndt2d_robust_*: a third prefix on the same object, for the reason given at the
 * preconditioner's).  A loss rho is applied to chosen constraints; with s_c = |r_c|^2, a scale
 * a > 0 and b = a^2 (csrc/posegraph/ndt2d_posegraph_loss.h; Ceres's HuberLoss and CauchyLoss):
 *     "trivial" (default)  rho = s                  rho' = 1                    rho'' = 0
 *     "huber"    s <= b: as trivial; otherwise, q = sqrt(s):
 *                          rho = 2 a q - b          rho' = max(DBL_MIN, a / q)  rho'' = -rho' / (2 s)
 *     "cauchy"   u = 1 + s / b:
 *                          rho = b log(u)           rho' = max(DBL_MIN, 1 / u)  rho'' = -rho'^2 / b
 * A constraint the loss is not applied to has rho = s.  The cost of a job is then
 *     F = 1/2 sum rho(s_c) over its enabled constraints,
 * and, both losses having rho'' <= 0 (Ceres's corrector applies no second-order term there), the
 * linearisation is plain reweighting:
 *     g = sum rho'_c J_c^T r_c          H = sum rho'_c J_c^T J_c
 * This g is the exact gradient of F; H is positive semidefinite because rho' > 0.  Everything the
 * solver above is said to do it does on these: D = diag(H) of the reweighted H, the gain ratio on the
 * robust F, the noise rule, the stop rules (|g|_inf of this g, F the robust cost), the record.
 * "chain"'s band is the band of the reweighted H + lambda D: a constraint's off-diagonal block
 * carries its rho'_c.  rho'_c is evaluated once per linearisation, at the accepted point, the same
 * bits wherever it is used; a job's workspace on the device gains m doubles for it.  Under a loss
 * cost_out, initial_cost and final_cost are the robust F, while chi2_out stays |r_c|^2: the weight
 * of a constraint at the solution is rho'(chi2 at the end), ndt2d_robust_rho on the host (a
 * verdict on each constraint from one solve; no policy is applied).  What a result depends on is
 * the graph, the job's mask, the loss with its scale and selection, and the parameters; the
 * determinism above holds.  With "trivial" the kernels are the ones without a loss, bit for bit.
 *   ndt2d_robust_rho       rho3_out = {rho, rho', rho''} of `kind` at `scale` and s; a pure host
 *              function.  NDT2D_ERR_INVALID: an unknown kind, a scale that is not finite and > 0
 *              (whatever the kind), an s that is negative or not finite, a NULL rho3_out.
 *   ndt2d_robust_set_loss / ndt2d_robust_loss   the loss of the object; kept across set_graph.
 *              "trivial" ignores the scale (and keeps the one set before).  Anything invalid (as for
 *              ndt2d_robust_rho): NDT2D_ERR_INVALID, the setting in place stays.  ndt2d_robust_loss
 *              returns the kind ("" for NULL) and, if scale_out is not NULL, the scale (1 at first).
 *   ndt2d_robust_select    robust[m] bytes: the constraints the loss applies to (non-zero: applied);
 *              NULL: every constraint.  m must be the graph's m (NDT2D_ERR_INVALID otherwise); before
 *              set_graph: NDT2D_ERR_STATE.  set_graph resets the selection to every constraint.
 *
 * Marginal covariances (ndt2d_marginals_*: a fourth prefix on the same object, for the same
 * reason).  How certain the poses are: block columns of the inverse of the matrix the solver
 * linearises, of the object's graph under a job's mask, the object's weighting and loss, at poses
 * x -- the graph's own (poses NULL), or one [n][3] set per job, so that solve's poses_out goes
 * straight in.
 *     The matrix.  H = sum rho'_c J_c^T J_c over the job's enabled constraints, exactly the H above,
 * rho' evaluated at x (1 without a loss).  F: the job's free nodes -- not the fixed one, and with at
 * least one enabled constraint.  The result is the inverse of
 *     H_FF + damping clamp(diag H_FF),      damping >= 0, the clamp the solver's [1e-6, 1e32].
 * With damping = 0 this is Sigma = H_FF^-1: under "information" the Gauss-Newton covariance of the
 * poses (H is then sum rho' J^T information J), under "reference" the inverse of the reference's own
 * quirky H (J^T L^T L J), which is a covariance only where every L is diagonal.
 *     The outputs.  For each job and each of Q query nodes q the block column Sigma[:, q]: n blocks
 * of 3 x 3, row-major; the blocks of nodes not in F are zero.
 *     blocks_out[K][Q][Q][9]   always: block (i, j) is the rows of node q_i in the column of q_j, as
 *                              computed, not symmetrised.
 *     columns_out[K][Q][n][9]  optional (NULL: not read back).
 *     records_out[K][Q][NDT2D_MARGINALS_RECORD_DOUBLES] = {status, cg_iterations, |r|_2 of the
 *                              node's columns 0, 1, 2 at the end}.
 * Duplicate queries are legal.  A query on the fixed node or on a node with no enabled constraint
 * gets a zero column, residuals 0 and NDT2D_MARGINALS_NOT_FREE.
 *     The solve.  Each of the three unit vectors of a query node by preconditioned conjugate
 * gradients from 0, with the object's preconditioner: "jacobi", or "chain" with the band factored
 * once per job (the damping does not change; a pivot that is not positive definite leaves the job
 * to the Jacobi blocks, as in the solver).  The three columns of a node advance in lockstep in one
 * workgroup; cg_iterations is the iterations of the last of them to stop.  A column stops when its
 * recurrence residual has |r|_2 <= tolerance, tested after each iteration (the right-hand side has
 * norm 1; tolerance > 0), when p . H p <= 0 or a value is not finite (BREAKDOWN), or at
 * max_cg_iterations (0: the solver's cap, min(3 n + 16, 8192)); it is then frozen.  The status of a
 * query is BREAKDOWN if a column broke down, else CG_CAP if one met the cap, else CONVERGED.  A
 * query in a component not joined to the fixed pose has no inverse at damping = 0: it is promised
 * only "not CONVERGED", and its columns stay as the iteration left them.
 *     Determinism.  The solver's rules: no atomics, gathers in ascending constraint index, fixed
 * reduction trees.  A column's bits depend on the graph, the mask, the poses, the settings and its
 * node -- not on the other queries, the other jobs, their order, the chunking or the run.
 *     The workspace on the device is made at the first call (create's arguments are what they
 * were) and freed by destroy: per job of a chunk a solver workspace (41 doubles a node, 83 under
 * "chain", m more under a loss) plus one, per workgroup of a chunk 45 doubles a node, 54 under "chain".
 * The pairs run in chunks of at most max_jobs pairs.  A pair is one workgroup with its three columns
 * in lockstep, or, while three workgroups a pair still find a compute unit of the device each, three
 * workgroups with one column each -- the same operations per column, the same bits.  Neither the
 * chunking nor the form changes an output.
 *   ndt2d_marginals_columns   NDT2D_ERR_INVALID before anything runs: a NULL object; NULL nodes,
 *              blocks_out or records_out with Q > 0; a node index >= n (the message names it); a
 *              non-finite pose in poses ("job k pose i"); a negative or non-finite damping; a
 *              tolerance that is not finite and > 0.  Q == 0 or n_jobs == 0: NDT2D_OK, nothing done.
 *              Before set_graph: NDT2D_ERR_STATE.  set_timing / last_ms cover its two launches.
 *   ndt2d_marginals_relative  a pure host function (csrc/posegraph/ndt2d_posegraph_relative.h): the
 *              predicted transform of b in a's frame (R_a^T (p_b - p_a), theta_b - theta_a) and its
 *              covariance [A B] sym(joint) [A B]^T with the A and B above and joint[2][2][9] =
 *              {aa, ab, ba, bb} (blocks_out of the call with nodes = {a, b}), sym(J) = (J + J^T) / 2.
 *              A zero aa block means a is held.  NDT2D_ERR_INVALID: a NULL or non-finite argument.
 *   ndt2d_marginals_distance  a pure host function: e = meas - pred, the heading through Normalize,
 *              S = covariance_pred + covariance_meas, d2_out = e^T S^-1 e.  NDT2D_ERR_INVALID: a NULL
 *              or non-finite argument, or S not positive definite by the Cholesky above (only its
 *              lower triangle is read).  A verdict, no policy: no accept rule anywhere changes. */
#define NDT2D_MARGINALS_RECORD_DOUBLES 5
#define NDT2D_MARGINALS_CONVERGED 0
#define NDT2D_MARGINALS_CG_CAP 1
#define NDT2D_MARGINALS_BREAKDOWN 2
#define NDT2D_MARGINALS_NOT_FREE 3
#define NDT2D_POSEGRAPH_RECORD_DOUBLES 6
#define NDT2D_POSEGRAPH_CONVERGED_GRADIENT 0
#define NDT2D_POSEGRAPH_CONVERGED_COST 1
#define NDT2D_POSEGRAPH_CONVERGED_STEP 2
#define NDT2D_POSEGRAPH_MAX_ITERATIONS 3
#define NDT2D_POSEGRAPH_FAILED 4
typedef struct ndt2d_posegraph ndt2d_posegraph;
int ndt2d_posegraph_create(ndt2d_handle h, size_t max_nodes, size_t max_constraints, size_t max_jobs,
                           ndt2d_posegraph ** out);
int ndt2d_posegraph_destroy(ndt2d_posegraph * posegraph);
const char * ndt2d_posegraph_last_error(ndt2d_posegraph * posegraph);
int ndt2d_posegraph_set_graph(ndt2d_posegraph * posegraph, const double * poses_xyt, size_t n,
                              const uint32_t * begin, const uint32_t * end, const double * transform,
                              const double * information, size_t m, size_t fixed);
int ndt2d_posegraph_set_weighting(ndt2d_posegraph * posegraph, const char * weighting);
const char * ndt2d_posegraph_weighting(ndt2d_posegraph * posegraph);
int ndt2d_pose_graph_set_preconditioner(ndt2d_posegraph * posegraph, const char * preconditioner);
const char * ndt2d_pose_graph_preconditioner(ndt2d_posegraph * posegraph);
int ndt2d_posegraph_evaluate(ndt2d_posegraph * posegraph, const uint8_t * enabled, size_t n_jobs,
                             double * cost_out, double * chi2_out, double * residuals_out);
int ndt2d_posegraph_solve(ndt2d_posegraph * posegraph, const uint8_t * enabled, size_t n_jobs,
                          uint32_t max_iterations, double gradient_tolerance,
                          double function_tolerance, double parameter_tolerance, double * poses_out,
                          double * records_out, double * chi2_out);
int ndt2d_posegraph_set_timing(ndt2d_posegraph * posegraph, int enabled);
int ndt2d_posegraph_last_ms(ndt2d_posegraph * posegraph, float * kernel_ms, float * fetch_ms);
int ndt2d_robust_rho(const char * kind, double scale, double s, double * rho3_out);
int ndt2d_robust_set_loss(ndt2d_posegraph * posegraph, const char * kind, double scale);
const char * ndt2d_robust_loss(ndt2d_posegraph * posegraph, double * scale_out);
int ndt2d_robust_select(ndt2d_posegraph * posegraph, const uint8_t * robust, size_t m);
int ndt2d_marginals_columns(ndt2d_posegraph * posegraph, const uint8_t * enabled, size_t n_jobs,
                            const double * poses, const uint32_t * nodes, size_t n_nodes,
                            double damping, double tolerance, uint32_t max_cg_iterations,
                            double * blocks_out, double * columns_out, double * records_out);
int ndt2d_marginals_relative(const double * pose_a, const double * pose_b, const double * joint,
                             double * transform_out, double * covariance_out);
int ndt2d_marginals_distance(const double * transform_pred, const double * covariance_pred,
                             const double * transform_meas, const double * covariance_meas,
                             double * d2_out);

/* Dense covariance (ndt2d_covariance_*: an object of its own beside an ndt2d_posegraph, which it
 * refers to and is destroyed before).  For each job -- a mask over the pose graph's graph, as
 * everywhere above -- the 3 x 3 diagonal block of EVERY node and the blocks of chosen (a, b) pairs of
 *     Sigma = (H_FF + damping clamp(diag H_FF))^-1,
 * the matrix of "Marginal covariances": the same H (sum rho'_c J_c^T J_c over the job's enabled
 * constraints), the pose graph's weighting and loss as they are at the call, the same free set F
 * and clamp [1e-6, 1e32], at the graph's poses (poses NULL) or at one [n][3] set per job.  The cost
 * does not depend on the number of closures: A = H_FF + damping clamp(diag) is assembled densely
 * (d = 3 n; a node not in F and the padding to whole panels of 48 keep the identity's rows and
 * columns), factored A = L L^T by a blocked right-looking Cholesky without pivoting (panels of 48;
 * the trailing update on the FP64 matrix cores, lower blocks only), T = L^-1 is formed by the same
 * panels, and each asked block is Sigma_ab = sum over k >= 3 max(a, b) of T[k, a]^T T[k, b].
 *     The outputs.  diagonal_out[K][n][9]: node i's block, row-major, symmetric bit for bit.
 * pairs_out[K][P][9]: for pairs[P][2] = {a, b} the rows of node a in the columns of node b,
 * row-major; duplicates and a == b are legal; pairs and pairs_out may be NULL with n_pairs == 0.
 * Blocks are as computed, nothing is symmetrised afterwards: every block, whichever way round it is
 * asked, is summed from the one lower-triangular factor T (only the lower triangle of A is
 * assembled and factored), (a, b) and (b, a) by the same products in the same order, so they are
 * transposes of each other bit for bit.  A block with a node not in F is zero.
 * records_out[K][NDT2D_COVARIANCE_RECORD_DOUBLES] = {status, the first failing unknown (3 node + j)
 * or -1, the pivot ratio}: the smallest, over the unknowns of F, of (the pivot before its square
 * root) / (that unknown's diagonal entry of A); an unknown not in F has the ratio 1, which is also
 * the largest a ratio can be.
 *     Not positive definite.  A pivot <= 0 or not finite: NDT2D_COVARIANCE_NOT_POSITIVE_DEFINITE,
 * the job's blocks are zero, the pivot ratio is the smallest up to that pivot, and the other jobs
 * of the call are untouched.  A singular matrix (a component not joined to the fixed pose at
 * damping = 0) is promised only: NOT_POSITIVE_DEFINITE, or OK with a pivot ratio at rounding level
 * (about (d + 1) eps).
 *     Determinism.  No atomics, no split sums: a block of A has one writer that walks the node's
 * constraints in ascending constraint index, every element of the factorisation is summed over k in
 * ascending order by one thread or one wave, a block of Sigma by a fixed tree.  A job's bits depend
 * on the graph, the mask, the poses, the settings and the pair list -- not on the other jobs, the
 * chunking, workspace_bytes or the run.
 *     Memory.  Per job of a chunk two matrices of padded(d)^2 doubles (A then L; the identity then
 * T), padded(d) = d rounded up to a multiple of 48, plus padded(d) + 3 n doubles.  The workspace is
 * allocated at the first compute (what the call's largest chunk needs, never more than
 * workspace_bytes) and freed by destroy.  The jobs of a chunk share every launch; a chunk holds
 * min(the pose graph's max_jobs, workspace_bytes / bytes per job) jobs.
 *   create    NDT2D_ERR_INVALID: a NULL posegraph or out, workspace_bytes == 0.
 *   compute   NDT2D_ERR_INVALID before anything runs, the message names the item: a NULL object
 *             (no message), NULL diagonal_out or records_out, NULL pairs or pairs_out with
 *             n_pairs > 0, a pair index >= n ("pair q names node i"), a non-finite pose ("job k pose
 *             i"), a negative or non-finite damping, more than 21,840 poses, a graph of which one
 *             job does not fit workspace_bytes (the message gives the bytes a job needs).
 *             n_jobs == 0: NDT2D_OK, nothing done.  Before set_graph: NDT2D_ERR_STATE.
 *   set_timing / last_ms   HIP events around the launches and the read-back of the last chunk. */
#define NDT2D_COVARIANCE_RECORD_DOUBLES 3
#define NDT2D_COVARIANCE_OK 0
#define NDT2D_COVARIANCE_NOT_POSITIVE_DEFINITE 1
typedef struct ndt2d_covariance ndt2d_covariance;
int ndt2d_covariance_create(ndt2d_posegraph * posegraph, size_t workspace_bytes,
                            ndt2d_covariance ** out);
int ndt2d_covariance_destroy(ndt2d_covariance * covariance);
const char * ndt2d_covariance_last_error(ndt2d_covariance * covariance);
int ndt2d_covariance_compute(ndt2d_covariance * covariance, const uint8_t * enabled, size_t n_jobs,
                             const double * poses, double damping, const uint32_t * pairs,
                             size_t n_pairs, double * diagonal_out, double * pairs_out,
                             double * records_out);
int ndt2d_covariance_set_timing(ndt2d_covariance * covariance, int enabled);
int ndt2d_covariance_last_ms(ndt2d_covariance * covariance, float * kernel_ms, float * fetch_ms);

/* Direct solve (ndt2d_direct_*: an object of its own beside an ndt2d_posegraph, which it refers to
 * and is destroyed before).  A second way to solve the problem of "Pose graph" and "Robust losses":
 * the same residual, weighting, losses, cost F, Jacobians, H, g and D = clamp(diag H) to
 * [1e-6, 1e32], by the same device functions, and the same Levenberg-Marquardt rules -- but the
 * linear step is exact: A = H_FF + lambda D is assembled densely and factored A = L L^T by the blocked
 * Cholesky of "Dense covariance" (the factor's launches only, no inverse), and delta solves
 * L L^T delta = -g by two substitutions.  An iteration's cost does not depend on the number of
 * closures, and its launches span the chip.  ndt2d_posegraph_solve stays the default solver.
 *     ndt2d_direct_solve takes ndt2d_posegraph_solve's arguments with their meanings: enabled[K][m]
 * or NULL, poses_out[K][n][3], an optional chi2_out[K][2][m] (at the start and at the end), the pose
 * graph's weighting and loss as they are at the call, the same free set -- a node that cannot move
 * (the fixed one, or without an enabled constraint) keeps its bits, -0.0 included.
 *     The LM rules.  lambda_0 = 1e-4, nu = 2.  With dF = F - F_trial and the model's decrease
 * predicted = 1/2 (lambda delta^T D delta - g^T delta) (an exact step leaves no residual term), a
 * step is accepted when F_trial is finite, predicted > 0 and the gain ratio dF / predicted is above
 * 1e-3 -- or, where |dF| <= 256 eps F, by the model alone.  Accepted: lambda *= max(1/3,
 * 1 - (2 gain - 1)^3), under the noise rule 1/3, nu = 2.  Rejected: lambda *= nu, nu *= 2.  lambda
 * stays within [1e-32, 1e32].  A factorisation that fails (a pivot <= 0 or not finite) counts as a
 * rejected step: lambda and nu move as on a rejection and no trial point is evaluated.  The four
 * stop rules and the status values are NDT2D_POSEGRAPH_*, evaluated where the CG solver evaluates
 * them (the step rule before the trial's cost, the gradient and the cost rule behind an accepted
 * step); an iteration is counted whether its step is accepted or not.
 *     records_out[K][NDT2D_DIRECT_RECORD_DOUBLES] = {status, iterations, rejected steps (failed
 * factorisations among them), factorisations that failed, initial_cost, final_cost, final |g|_inf,
 * the smallest pivot ratio of the last successful factorisation in "Dense covariance"'s definition
 * (1 before the first)}.  initial_cost is ndt2d_posegraph_evaluate's F bit for bit.  A start cost
 * that is not finite: NDT2D_POSEGRAPH_FAILED and the start poses.  m = 0 or n = 1: nothing moves,
 * NDT2D_POSEGRAPH_CONVERGED_GRADIENT.
 *     An iteration of a chunk is a fixed list of launches -- the assembly at each job's own lambda,
 * the factor's launches, one workgroup per job for the substitutions, one for the step -- after
 * which the host reads the jobs' states back (one small read-back per LM iteration) and stops when
 * no job is iterating or after max_iterations.  No waiting on the device.  The stream is the
 * context's current one.  A job that has stopped is left alone: its poses and record do not change.
 *     Determinism.  No atomics, every sum in a fixed order.  A job's bits depend on the graph, the
 * mask, the settings and the tolerances -- not on the other jobs, the chunking, workspace_bytes,
 * whether other jobs of the call have already stopped, or the run.
 *     Memory.  Per job of a chunk ONE matrix of padded(d)^2 doubles (A, then L; d = 3 n, padded(d)
 * = d rounded up to a multiple of 48), 2 padded(d) + 3 n doubles beside it (the diagonal, the
 * substitutions' vector, cos / sin / free flag per node), the CG solver's node arrays (41 n
 * doubles, m more under a loss) and 16 doubles of state: 8 (padded(d)^2 + 2 padded(d) + 44 n
 * [+ m] + 16) bytes.  The workspace is allocated at the first solve (what the call's largest chunk
 * needs, never more than workspace_bytes) and freed by destroy; a chunk holds min(the pose graph's
 * max_jobs, workspace_bytes / bytes per job) jobs.
 *   create    NDT2D_ERR_INVALID: a NULL posegraph or out, workspace_bytes == 0.
 *   solve     NDT2D_ERR_INVALID before anything runs: a NULL object (no message), NULL poses_out or
 *             records_out, a negative or non-finite tolerance, more than 21,840 poses, a graph of
 *             which one job does not fit workspace_bytes (the message gives the bytes a job needs).
 *             n_jobs == 0: NDT2D_OK, nothing done.  Before set_graph: NDT2D_ERR_STATE.
 *   set_timing / last_ms   HIP events around the last chunk's iterations (the read-backs between
 *             them included) and its final read-back. */
#define NDT2D_DIRECT_RECORD_DOUBLES 8
typedef struct ndt2d_direct ndt2d_direct;
int ndt2d_direct_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_direct ** out);
int ndt2d_direct_destroy(ndt2d_direct * direct);
const char * ndt2d_direct_last_error(ndt2d_direct * direct);
int ndt2d_direct_solve(ndt2d_direct * direct, const uint8_t * enabled, size_t n_jobs,
                       uint32_t max_iterations, double gradient_tolerance,
                       double function_tolerance, double parameter_tolerance, double * poses_out,
                       double * records_out, double * chi2_out);
int ndt2d_direct_set_timing(ndt2d_direct * direct, int enabled);
int ndt2d_direct_last_ms(ndt2d_direct * direct, float * kernel_ms, float * fetch_ms);

/* Sparse solve (ndt2d_sparse_*: an object of its own beside an ndt2d_posegraph, which it refers to
 * and is destroyed before).  A third way to solve the problem of "Pose graph" and "Robust losses",
 * for the graphs a mapping session builds: a chain along the node order plus closures.  The problem
 * is "Direct solve"'s term for term -- the residual, the weighting, the losses, F, the Jacobians,
 * H = J^T J reweighted by rho', g, D = clamp(diag H_FF), A = H_FF + lambda D -- and so are the LM
 * rules, bit for bit in their logic: lambda_0, nu, the gain ratio, the noise rule, the four stop
 * rules, the statuses, predicted = 1/2 (lambda delta^T D delta - g^T delta), a failed factorisation
 * counts as a rejected step.  Only the linear step A delta = -g is computed differently: its cost
 * is O(n) for the chain plus O(s^3) for the s nodes closures touch, and no 3n x 3n matrix exists.
 *     Separators.  A constraint is a chain edge when |begin - end| == 1, every other one a closure
 * edge.  The separators are the nodes that are an end of at least one closure edge of the GRAPH,
 * whatever the masks: the layout is one per graph, shared by the K jobs, and a job's bits do not
 * depend on the other jobs' masks.  The fixed node and the nodes a job's mask leaves without a
 * constraint are not unknowns, as in "Direct solve"; they only cut the chain.  The interior nodes
 * are all the others, in node order.  ndt2d_sparse_layout reports the two counts.
 *     The step.  The interior block A_ii is ONE block-tridiagonal SPD system over the interior
 * nodes in node order (the coupling between two interior nodes that are not consecutive, or whose
 * chain edge is off or absent, is zero; a principal submatrix of an SPD matrix is SPD, so block
 * cyclic reduction without pivoting applies for any mask), factored by "Pose graph"'s chain
 * reduction, all segments at once.  A_is has at most two 3 x 3 blocks per interior node -- to the
 * separator directly before it and to the one directly after it -- so Z = A_ii^-1 A_is is six
 * right-hand-side columns through the same reduction, and a seventh is y = A_ii^-1 (-g_i).  Then
 * S = A_ss - A_si Z (a thread per separator writes its own block row; no atomics) in a dense
 * padded(3 s)^2 matrix, factored S = L L^T by "Dense covariance"'s blocked Cholesky (the factor's
 * launches only), S delta_s = -g_s - A_si y by "Direct solve"'s substitution, and
 * delta_i = y_i - Z_left[i] delta_left(i) - Z_right[i] delta_right(i).  A non-positive pivot met
 * by the reduction or by S's Cholesky is a failed factorisation.  With s = 0 nothing dense is
 * launched.
 *     ndt2d_sparse_solve takes ndt2d_direct_solve's arguments with their meanings, and
 * records_out[K][NDT2D_DIRECT_RECORD_DOUBLES] has the direct solve's: the pivot ratio is S's (of the
 * Schur complement against its own diagonal; 1 when s = 0), the failed factorisations count a
 * failure of the reduction and a failure of S alike.  initial_cost is ndt2d_posegraph_evaluate's F
 * bit for bit; a node that cannot move keeps its bits, -0.0 included.
 *     An iteration of a chunk is a fixed list of launches -- S's fill, the band's assembly at each
 * job's own lambda, one workgroup per job for the reduction, the Schur terms, S's factor, one
 * workgroup per job for the substitution, the expansion, one for the step -- after which the host
 * reads the jobs' states back (one small read-back per LM iteration) and stops when no job is
 * iterating or after max_iterations.  No waiting on the device.  The stream is the context's
 * current one.  A job that has stopped is left alone.
 *     Determinism.  No atomics, every sum in a fixed ascending order, fixed reduction trees.  A
 * job's bits depend on the graph, its mask, the settings and the tolerances -- not on the other
 * jobs, the chunking, workspace_bytes or the run.
 *     Memory.  Per job of a chunk 90 doubles per interior node (the reduction's D, U, L, P, the
 * seven columns, Z and y, the couplings to the separators), padded(3 s)^2 + 2 padded(3 s) + 6 s for
 * the separators, the CG solver's node arrays (41 n doubles, m more under a loss) and 17 doubles of
 * state: 8 (90 n_i + padded(3 s)^2 + 2 padded(3 s) + 6 s + 41 n [+ m] + 17) bytes, 1 KiB a pose
 * where closures are few.  The workspace is allocated at the first solve (what the call's largest
 * chunk needs, never more than workspace_bytes) and freed by destroy.
 *   create    NDT2D_ERR_INVALID: a NULL posegraph or out, workspace_bytes == 0.
 *   solve     NDT2D_ERR_INVALID before anything runs: a NULL object (no message), NULL poses_out or
 *             records_out, a negative or non-finite tolerance, more than 21,840 separators, a graph
 *             of which one job does not fit workspace_bytes (the message gives the bytes a job
 *             needs).  n_jobs == 0: NDT2D_OK, nothing done.  Before set_graph: NDT2D_ERR_STATE.
 *   layout    the separators and the interior nodes of the graph in place.  NDT2D_ERR_INVALID: a
 *             NULL object or output; before set_graph NDT2D_ERR_STATE.
 *   set_timing / last_ms   as "Direct solve"'s. */
typedef struct ndt2d_sparse ndt2d_sparse;
int ndt2d_sparse_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_sparse ** out);
int ndt2d_sparse_destroy(ndt2d_sparse * sparse);
const char * ndt2d_sparse_last_error(ndt2d_sparse * sparse);
int ndt2d_sparse_solve(ndt2d_sparse * sparse, const uint8_t * enabled, size_t n_jobs,
                       uint32_t max_iterations, double gradient_tolerance,
                       double function_tolerance, double parameter_tolerance, double * poses_out,
                       double * records_out, double * chi2_out);
int ndt2d_sparse_layout(ndt2d_sparse * sparse, size_t * n_separators, size_t * n_interior);
int ndt2d_sparse_set_timing(ndt2d_sparse * sparse, int enabled);
int ndt2d_sparse_last_ms(ndt2d_sparse * sparse, float * kernel_ms, float * fetch_ms);

/* Sparse covariance (ndt2d_sparsecov_*: an object of its own beside an ndt2d_posegraph, which it
 * refers to and is destroyed before).  "Dense covariance"'s call for the graphs "Sparse solve" is
 * for: per job the 3 x 3 diagonal block of EVERY node and the blocks of chosen (a, b) pairs of
 *     Sigma = (H_FF + damping clamp(diag H_FF))^-1,
 * the matrix of "Dense covariance" -- the same H, weighting, loss, free set F and clamp, at the
 * graph's poses (poses NULL) or at one [n][3] set per job -- in O(n) + O(s^3) for s separators and
 * without a dense 3n x 3n matrix.  The arguments and the outputs are ndt2d_covariance_compute's, so
 * that a caller can switch.
 *     The factorisation is "Sparse solve"'s linear step at lambda = damping, launched as it is there:
 * the interior block A_ii by the block cyclic reduction, Z = A_ii^-1 A_is by six columns through it,
 * S = A_ss - A_si Z factored S = L L^T by "Dense covariance"'s blocked Cholesky, here followed by its
 * inversion T = L^-1.  With i for interior and s for separator the blocks of the inverse are
 *     Sigma_ss = S^-1,   Sigma_is = -Z Sigma_ss,   Sigma_ii = A_ii^-1 + Z Sigma_ss Z^T.
 * An interior node k couples to the separator before it (u) and the one after it (w) only, so
 *     Sigma_kk = G_kk + [Zl_k Zr_k] [Sigma_uu Sigma_uw; Sigma_wu Sigma_ww] [Zl_k Zr_k]^T,  G = A_ii^-1,
 * a sum of two positive semidefinite terms.  The blocks of S^-1 are sums over T's rows, as the dense
 * call's.  The diagonal blocks G_kk come from a selected inversion down the levels the reduction has
 * factored: from the root's G_00 = P_0, for a node i eliminated at stride sigma into lo = i - sigma
 * and hi = i + sigma, G_i,lo = -P_i (L_i^T G_lo,lo + U_i G_hi,lo), G_i,hi likewise, and
 * G_i,i = P_i - (G_i,lo L_i + G_i,hi U_i^T) P_i: 24 doubles a node, one barrier a level.  A pair's
 * block is Sigma_ab = C_a Sigma_{N(a), N(b)} C_b^T over the at most two separators each node reaches
 * (C = the identity for a separator, -Zl and -Zr for an interior node), plus G_ab where both are
 * interior nodes of one segment and a != b; G_ab is taken from a three-column solve A_ii^-1 E_b
 * through the reduction, one pass per distinct such b.
 *     The outputs.  diagonal_out[K][n][9] and pairs_out[K][P][9] with the dense call's meaning and
 * layout: row-major, pairs[P][2] = {a, b} the rows of node a in the columns of node b, duplicates and
 * a == b legal ((a, a) is the diagonal block), pairs and pairs_out may be NULL with n_pairs == 0.  A
 * diagonal block is symmetric bit for bit (its upper triangle is computed and mirrored).  The block
 * of (a, b) with a > b is returned as the transpose of the block computed for (b, a): the two are
 * transposes bit for bit.  A block with a node not in F is zero.
 * records_out[K][NDT2D_COVARIANCE_RECORD_DOUBLES] = {status, stage, the pivot ratio}: status is
 * NDT2D_COVARIANCE_OK or NDT2D_COVARIANCE_NOT_POSITIVE_DEFINITE; stage is 0 for none, 1 for a pivot
 * of the reduction, 2 for a pivot of S; the pivot ratio is S's, 1 when s = 0, as in "Sparse solve".
 *     Not positive definite.  A job that fails has zero blocks; the other jobs of the call are
 * untouched.  The reduction keeps no pivot ratio: for a singular matrix (a component not joined to
 * the fixed pose at damping = 0) nothing is promised beyond a clean return with either status.
 *     Determinism.  No atomics, every sum in a fixed order.  A job's diagonal does not depend on the
 * pair list, the other jobs, the chunking, workspace_bytes or the run; a pair's block does not
 * depend on the other pairs.
 *     Memory.  Per job of a chunk "Sparse solve"'s doubles, 24 more per interior node, a second
 * padded(3 s)^2 matrix (T), and 9 doubles per block of S^-1 that is wanted (2 s - 1, and at most four
 * more per pair) and per pair: 8 (114 n_i + 2 padded(3 s)^2 + 2 padded(3 s) + 6 s + 9 blocks +
 * 9 P + 41 n [+ m] + 17) bytes.  The workspace is allocated at the first compute (what the call's
 * largest chunk needs, never more than workspace_bytes) and freed by destroy.  The jobs of a chunk
 * share every launch.
 *   create    NDT2D_ERR_INVALID: a NULL posegraph or out, workspace_bytes == 0.
 *   compute   NDT2D_ERR_INVALID before anything runs, the message names the item: a NULL object
 *             (no message), NULL diagonal_out or records_out, NULL pairs or pairs_out with
 *             n_pairs > 0, a pair index >= n ("pair q names node i"), a non-finite pose ("job k pose
 *             i"), a negative or non-finite damping, more than 21,840 separators, a graph of which
 *             one job does not fit workspace_bytes (the message gives the bytes a job needs).
 *             n_jobs == 0: NDT2D_OK, nothing done.  Before set_graph: NDT2D_ERR_STATE.
 *   last_error   of a NULL object: "null sparsecov".
 *   set_timing / last_ms   HIP events around the launches and the read-back of the last chunk. */
typedef struct ndt2d_sparsecov ndt2d_sparsecov;
int ndt2d_sparsecov_create(ndt2d_posegraph * posegraph, size_t workspace_bytes,
                           ndt2d_sparsecov ** out);
int ndt2d_sparsecov_destroy(ndt2d_sparsecov * sparsecov);
const char * ndt2d_sparsecov_last_error(ndt2d_sparsecov * sparsecov);
int ndt2d_sparsecov_compute(ndt2d_sparsecov * sparsecov, const uint8_t * enabled, size_t n_jobs,
                            const double * poses, double damping, const uint32_t * pairs,
                            size_t n_pairs, double * diagonal_out, double * pairs_out,
                            double * records_out);
int ndt2d_sparsecov_set_timing(ndt2d_sparsecov * sparsecov, int enabled);
int ndt2d_sparsecov_last_ms(ndt2d_sparsecov * sparsecov, float * kernel_ms, float * fetch_ms);

/* Upload the beam endpoints of one scan, robot frame, already subsampled to
 * min(laser_max_beams, points.size()) points by the caller
 * (src/scan_matcher_ndt.cpp:95-96,110 / :165-166,171).  Beams are taken as given: finite,
 * within +-1e200 m (see "Points off the grid" at ndt2d_host_build_grid_ex). */
int ndt2d_set_beams(ndt2d_handle h, const double * beams_xy, size_t n_beams);

/* Upload the search lattice of matchScan.  dth[n_th] / dlin[n_lin] are the
 * values the reference's floating-point loops visit
 * (`for (dth = -angular_size_; dth < angular_size_; dth += angular_res_)`,
 * src/scan_matcher_ndt.cpp:103,117,119); cos_th/sin_th[n_th] are
 * cos/sin(scan_pose.theta + dth[i]) evaluated by the host libm (:106-107);
 * pose_x/pose_y = scan_pose.x/.y (:112,114). */
int ndt2d_set_search(ndt2d_handle h, double pose_x, double pose_y, const double * dth,
                     const double * cos_th, const double * sin_th, size_t n_th,
                     const double * dlin, size_t n_lin);

/* ndt2d_set_beams + ndt2d_set_search in one call: both travel in ONE staged copy (a
 * small search is a few tens of microseconds; every copy command costs ~3 us).
 * beams_xy == NULL: the n_beams beams the context already holds stay (the caller knows
 * they are this scan's: ndt2d_matcher_* compares), and the tables are only staged --
 * a small-lattice search takes them as kernel arguments, so such a call copies nothing. */
int ndt2d_set_search_beams(ndt2d_handle h, const double * beams_xy, size_t n_beams, double pose_x,
                           double pose_y, const double * dth, const double * cos_th,
                           const double * sin_th, size_t n_th, const double * dlin, size_t n_lin);

/* Result of one (possibly sharded) matchScan search,
 * src/scan_matcher_ndt.cpp:103-143.  Candidate flat index =
 * (i_theta * n_lin + i_x) * n_lin + i_y, the reference's loop order. */
typedef struct ndt2d_match_result
{
  double best_score;      /* raw best score = -NDT::likelihood (:127); 0.0 if none < 0 */
  uint64_t best_index;    /* flat index of the winner, NDT2D_NO_INDEX if none (:128) */
  double acc[10];         /* k00,k01,k02,k11,k12,k22, u0,u1,u2, s  (:137-140) */
  uint64_t n_candidates;  /* candidates evaluated by this call */
  /* 1: another candidate scored within the near-tie tolerance of the winner --
   * |difference| <= NDT2D_NEAR_TIE_REL * (the larger magnitude); the
   * kernels' scores differ from the CPU reference's in the last bits (device exp vs libm: a
   * relative error below 1e-13), so the two could come out in the other order there;
   * ndt2d_match_near_best lists such candidates and ndt2d_matcher_match_scan settles them with
   * the reference's own arithmetic.  0 proves that no other candidate lies that close. */
  uint64_t near_tie;
} ndt2d_match_result;
#define NDT2D_NEAR_TIE_REL 1.4551915228366852e-11   /* 2^-36 */

/* Number of doubles of the device-resident result record
 * {best_score, best_index (exact double, -1 if none; + 0.5 = near_tie, truncate), acc[10]}. */
#define NDT2D_MATCH_RECORD_DOUBLES 12

/* Evaluate the theta slab [th_begin, th_end) of the lattice (all n_lin x n_lin
 * translations of each theta).  Asynchronous on the context's stream.
 * d_scores (device pointer, optional): receives the raw score of every
 * candidate of the slab, slab-local flat order.  d_record (device pointer,
 * optional): receives the NDT2D_MATCH_RECORD_DOUBLES-double result record
 * (for a device-side all-reduce); the context always keeps its own copy. */
int ndt2d_match_launch(ndt2d_handle h, size_t th_begin, size_t th_end, double * d_scores,
                       double * d_record);
/* The same for the theta steps th_first, th_first + th_stride, ... (th_count of
 * them): one rank's share of a lattice whose theta axis is dealt out round-robin
 * (the cost of a step varies across the angular range, so contiguous slabs leave
 * the ranks unevenly loaded).  best_index is the flat index in the WHOLE lattice
 * ((i_theta * n_lin + i_x) * n_lin + i_y, the reference's visiting order
 * src/scan_matcher_ndt.cpp:103-119), d_scores is local: step k of this call first. */
int ndt2d_match_launch_strided(ndt2d_handle h, size_t th_first, size_t th_stride,
                               size_t th_count, double * d_scores, double * d_record);
/* Wait for the last ndt2d_match_launch and return its result.  (The final reduction
 * writes the record into host-coherent pinned memory and then raises a flag there; the
 * host spins on the flag, which returns ~4 us sooner than a stream synchronisation.) */
int ndt2d_match_fetch(ndt2d_handle h, ndt2d_match_result * out);
/* Search the slab [th_begin, th_end) keeping every candidate's score on the device, and list the
 * candidates that scored below 0 and within rel * |best| of the slab's best
 * (flat indices in the whole lattice, ascending).  *n_out = how many there are; when that exceeds
 * `capacity` the list holds the first `capacity`-or-fewer of them in visiting order (further passes
 * over the scores).  result_out (optional) = the slab's result.  Synchronous.  This is the slow path
 * behind a near_tie result: one more search plus one pass over its scores. */
int ndt2d_match_near_best(ndt2d_handle h, size_t th_begin, size_t th_end, double rel, uint64_t * index_out,
                          size_t capacity, size_t * n_out, ndt2d_match_result * result_out);
/* Searches launched and results fetched on this context so far: a layer that leaves a search
 * pending across calls (ndt2d_matcher_score_scan launches the next matchScan's search) checks
 * with these that nobody else launched or fetched on the context in between. */
int ndt2d_match_status(ndt2d_handle h, uint64_t * n_launched, uint64_t * n_fetched);
/* launch + fetch; h_scores (host pointer, optional) receives the slab scores. */
int ndt2d_match(ndt2d_handle h, size_t th_begin, size_t th_end, double * h_scores,
                ndt2d_match_result * out);

/* Batched ScanMatcherNDT::scorePoints (src/scan_matcher_ndt.cpp:156-178) =
 * the body of ParticleFilter::measure's loop (src/particle_filter.cpp:81-87):
 * scores[i] = sum_k -likelihood(T(pose_i) * beam_k) / n_beams for the beams of
 * ndt2d_set_beams.  d_* are device pointers; poses are {x, y, theta} triples.
 * d_stats (optional) receives NDT2D_POSE_STATS_DOUBLES doubles:
 * {sum w, sum w*x, sum w*y, sum w*cos(theta), sum w*sin(theta), sum w*x*x,
 *  sum w*x*y, sum w*y*y} with w = scores[i] (un-normalised), the sums
 * ParticleFilter::updateStatistics needs (src/particle_filter.cpp:166-200). */
#define NDT2D_POSE_STATS_DOUBLES 8
int ndt2d_score_poses_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                             double * d_scores, double * d_stats);
/* Host-pointer convenience: H2D poses, launch, D2H scores (+ stats).  Up to 8 poses
 * (scorePoints / scoreScan call it with ONE) take a block-per-pose kernel whose poses are
 * kernel arguments and whose scores land in host-coherent memory: one launch, no copy,
 * bit-identical scores.  Buffers from ndt2d_host_alloc are read / written by the kernel
 * in place (no copy is queued). */
int ndt2d_score_poses(ndt2d_handle h, const double * h_poses_xyt, size_t n_poses,
                      double * h_scores, double * h_stats);

/* ndt2d_set_beams + ndt2d_score_poses in one call.  Up to 8 poses and up to 208 beams
 * (a scoreScan with the plugin's default laser_max_beams = 100) travel as kernel
 * arguments: one launch, no copy at all, and the kernel leaves the beams in the context's
 * beam buffer for the calls that follow on the same scan.  Anything larger falls back to
 * the two calls. */
int ndt2d_score_poses_beams(ndt2d_handle h, const double * beams_xy, size_t n_beams,
                            const double * h_poses_xyt, size_t n_poses, double * h_scores);

/* The kernel-argument launch of ndt2d_score_poses_beams without the wait (<= 8 poses; beams_xy
 * with <= 208 beams, or NULL: the beams the context holds), and the wait.  Between the two the
 * caller may queue the search of the same scan -- the mapper calls scoreScan(scan) and then
 * matchScan(scan, ...) (reference src/ndt_mapper.cpp:514-515, 552-553), and a search queued
 * behind the scoring kernel starts when that ends instead of a host round trip later
 * (ndt2d_matcher_score_scan does this once it has seen the pair).  NDT2D_ERR_STATE when the
 * request is not a kernel-argument launch.  One launch may be pending per context. */
int ndt2d_score_poses_beams_launch(ndt2d_handle h, const double * beams_xy, size_t n_beams,
                                   const double * h_poses_xyt, size_t n_poses);
int ndt2d_score_fetch(ndt2d_handle h, double * h_scores);

/* ParticleFilter::updateStatistics (src/particle_filter.cpp:163-218) on the
 * device, from the (all-reduced) moment sums d_stats of ndt2d_score_poses_launch:
 * d_weights[n] are divided by the total weight in place (:171-174) and d_out
 * receives NDT2D_PF_RESULT_DOUBLES doubles {sum w, mean x, mean y, mean theta
 * (circular, :205), cov xx, cov xy, cov yy (:208-215), sum_i w_i *
 * shortest_angular_distance(theta_i, mean theta)^2 (:213-217, to be ADDED to the
 * caller's cov(2,2), which the reference never zeroes)}.  Device pointers,
 * asynchronous. */
#define NDT2D_PF_RESULT_DOUBLES 8
int ndt2d_pf_finalize_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                             double * d_weights, const double * d_stats, double * d_out);
/* The same in the form one device of a SHARDED particle set takes (ndt2d_matcher_create_multi,
 * host exchange): no copy and no stream synchronisation between the two halves of
 * ParticleFilter::measure.
 *   ndt2d_pose_sums_launch   = ndt2d_score_poses_launch whose eight moment sums
 *       (NDT2D_POSE_STATS_DOUBLES) also go to the context's host-coherent result block, behind
 *       a flag;  ndt2d_pose_sums_fetch spins on that flag and returns them (this device's row
 *       of the [n_dev, 8] table: the "total particle weight" exchange, src/particle_filter.cpp:166-174);
 *   ndt2d_pf_finalize_totals_launch = ndt2d_pf_finalize_launch with the TOTAL sums given as
 *       eight host values that travel as kernel arguments; its result lands in the host-coherent
 *       block as well: ndt2d_pf_result_read returns it once the caller has synchronised the
 *       stream (it does, behind its copy of the weights).
 * One such pair may be in flight per context. */
int ndt2d_pose_sums_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses, double * d_scores);
int ndt2d_pose_sums_fetch(ndt2d_handle h, double * sums_out);
int ndt2d_pf_finalize_totals_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n_poses,
                                    double * d_weights, const double * totals);
int ndt2d_pf_result_read(ndt2d_handle h, double * out);
/* Host-pointer convenience = ParticleFilter::measure for the beams of
 * ndt2d_set_beams: H2D particles, score, statistics, D2H normalised weights and
 * the NDT2D_PF_RESULT_DOUBLES result.  (From 131,072 particles the call is pipelined in pieces:
 * see ndt2d_set_pipeline_pieces for what that means for the last bits of the statistics.) */
int ndt2d_pf_measure(ndt2d_handle h, const double * h_poses_xyt, size_t n_poses,
                     double * h_weights, double * h_out);

/* ---- particle-filter steps either side of `measure` (particles stay in HBM) ----
 *
 * The reference draws three std::normal_distribution<float> values per particle
 * from an mt19937 seeded by std::random_device (include/ndt_2d/motion_model.hpp:
 * 63-64, particle_filter.hpp), i.e. not reproducibly.  Every call below takes the
 * draws either as d_noise = [n][3] float standard normals (device pointer), or
 * with d_noise == NULL from a counter-based stream: Philox4x32-10 keyed by
 * `seed`, counter (first_index + i, step) for particle i, Box-Muller.  In full: counter
 * words (index lo, index hi, step lo, step hi), key (seed lo, seed hi) give four words
 * w0..w3; the uniform of a word is the float  u(w) = fl((w >> 8) + 0.5) * 2^-24  with the
 * sum rounded to nearest even in float32 -- exactly (k + 0.5) 2^-24 for k = w >> 8 below
 * 2^23, an even multiple of 2^-24 from there, and 1.0f for k = 2^24 - 1: u lies in (0, 1];
 * r0 = sqrtf(-2 logf(u(w0))), r1 = sqrtf(-2 logf(u(w2))), angles the float products
 * a0 = 2 pi u(w1), a1 = 2 pi u(w3); the normals are (r0 cosf(a0), r0 sinf(a0), r1 cosf(a1)).
 * Every draw is finite, |z| <= sqrt(50 ln 2) = 5.887; u = 1 (probability 2^-24 per radius)
 * gives radius 0 and exactly zero normals.  The stream
 * depends on (seed, step, global particle index) only, so shards of a particle set
 * on different GPUs draw what the whole set would.  ndt2d_pf_noise_launch writes
 * that stream out (the same numbers a fused call uses). */
int ndt2d_pf_noise_launch(ndt2d_handle h, uint64_t seed, uint64_t step, uint64_t first_index,
                          size_t n, float * d_noise_out);
/* MotionModel::sample (src/motion_model.cpp:45-83) applied in place to
 * d_poses_xyt[n][3]; alphas5 = the model's {a1..a5} (motion_model.cpp:39-43;
 * a5 is unused by the reference too).  Asynchronous. */
int ndt2d_pf_motion_launch(ndt2d_handle h, double * d_poses_xyt, size_t n, double dx, double dy,
                           double dth, const double * alphas5, const float * d_noise,
                           uint64_t seed, uint64_t step, uint64_t first_index);
/* ParticleFilter::init sampling loop (src/particle_filter.cpp:53-65): poses
 * written as (float draw) widened to double, theta through normalize_angle. */
int ndt2d_pf_init_launch(ndt2d_handle h, double * d_poses_xyt, size_t n, double x, double y,
                         double theta, double sigma_x, double sigma_y, double sigma_theta,
                         const float * d_noise, uint64_t seed, uint64_t step,
                         uint64_t first_index);
/* The moment sums of updateStatistics (src/particle_filter.cpp:166-200) for given
 * weights (d_weights == NULL: uniform 1/n, as init assigns at :67): d_stats gets
 * NDT2D_POSE_STATS_DOUBLES doubles in ndt2d_score_poses_launch's layout, ready for
 * ndt2d_pf_finalize_launch (after an all-reduce when the set is sharded). */
int ndt2d_pose_moments_launch(ndt2d_handle h, const double * d_poses_xyt, size_t n,
                              const double * d_weights, double * d_stats);
/* Host-pointer convenience = ParticleFilter::update (src/particle_filter.cpp:
 * 71-76): motion model on h_poses_xyt in place (h_noise [n][3] or NULL = Philox),
 * then updateStatistics with h_weights (normalised in place) into h_out
 * (NDT2D_PF_RESULT_DOUBLES, see ndt2d_pf_finalize_launch). */
int ndt2d_pf_update(ndt2d_handle h, double * h_poses_xyt, size_t n, double dx, double dy,
                    double dth, const double * alphas5, const float * h_noise, uint64_t seed,
                    uint64_t step, double * h_weights, double * h_out);

/* ---- ParticleFilter::resample on the device (particles stay in HBM) ----
 *
 * The KLD draw-and-stop loop (src/particle_filter.cpp:91-137) as kernels.  For every
 * input the indices and the count are exactly what the host form ndt2d_kld_resample
 * (section 3, the parity reference) returns for the same particles, weights, uniforms
 * and parameters: the cumulative weights are summed in index order with one rounding
 * per add, a draw is libstdc++'s upper_bound bisection, the leaf count after draw i is
 * the number of distinct keys among draws 0..i, and the count kept is one more than the
 * first i whose size passes the stop test.  A resampler is an object of its own beside
 * the context: it owns its workspace (sized at creation) and a pinned word for the
 * count, launches on the context's current stream (ndt2d_set_stream), and must be
 * destroyed before ndt2d_destroy(h).  One launch may be in flight per resampler. */
typedef struct ndt2d_resampler ndt2d_resampler;
/* n_capacity: the most particles a launch may draw from (1 .. 2^32-1);
 * max_particles_capacity: the largest max_particles of a launch (up to 2^30). */
int ndt2d_resampler_create(ndt2d_handle h, size_t n_capacity, size_t max_particles_capacity,
                           ndt2d_resampler ** out);
int ndt2d_resampler_destroy(ndt2d_resampler * r);
const char * ndt2d_resampler_last_error(ndt2d_resampler * r);
/* The uniform stream a launch with d_uniforms == NULL uses, written to DEVICE
 * d_out[n]: Philox4x32-10 with key = seed and counter (first_index + i, step), the
 * convention of ndt2d_pf_noise_launch; u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, in
 * [0, 1) on the 2^-53 grid.  Asynchronous. */
int ndt2d_resample_uniforms_launch(ndt2d_resampler * r, uint64_t seed, uint64_t step,
                                   uint64_t first_index, size_t n, double * d_out);
/* The loop and the copy of the kept particles on DEVICE pointers, asynchronous:
 * d_particles_out[max_particles][3] and d_weights_out[max_particles] receive
 * in[p_j] for j < count (weights as they are: updateStatistics renormalises),
 * d_indices_out[max_particles] (or NULL) the p_j.  d_uniforms = [max_particles]
 * values in [0, 1) or NULL (the Philox stream of (seed, step), index 0 onwards).
 * leaf_size3 is a HOST pointer.  The outputs may not alias the inputs.  Refusals are
 * those of ndt2d_kld_resample, plus sizes beyond the created capacities
 * (NDT2D_ERR_INVALID); max_particles == 0 keeps nothing and is NDT2D_OK. */
int ndt2d_resample_launch(ndt2d_resampler * r, const double * d_particles_xyt,
                          const double * d_weights, size_t n, size_t min_particles,
                          size_t max_particles, double kld_err, double kld_z,
                          const double * leaf_size3, const double * d_uniforms, uint64_t seed,
                          uint64_t step, double * d_particles_out, double * d_weights_out,
                          uint32_t * d_indices_out);
/* Waits for the launch and returns the count kept (the gather read it from device
 * memory; no host round trip precedes it). */
int ndt2d_resample_fetch(ndt2d_resampler * r, size_t * n_out);
/* HIP events around the cumulative-weights kernel of each launch (the one serial
 * part: one dependent FP64 add per particle) on / off, and the last one's time. */
int ndt2d_resampler_set_timing(ndt2d_resampler * r, int enabled);
int ndt2d_resampler_cdf_ms(ndt2d_resampler * r, float * ms);
/* Host-pointer convenience with ndt2d_kld_resample's own arguments and a handle:
 * upload, launch, fetch, indices back. */
int ndt2d_pf_resample(ndt2d_handle h, const double * particles_xyt, const double * weights,
                      size_t n, size_t min_particles, size_t max_particles, double kld_err,
                      double kld_z, const double * leaf_size3, const double * uniforms,
                      size_t n_uniforms, uint32_t * indices_out, size_t * n_out);

/* ---- LaserScan -> Scan conversion on the device ----
 *
 * The loop of NdtMapper::laserCallback that turns a sensor_msgs/LaserScan into
 * the point list of an ndt_2d::Scan (src/ndt_mapper.cpp:385-453).  The message
 * fields keep their ROS types (float32); motion_* is `translation` (:386-389),
 * the odometry motion between the start and the end of the sweep; laser_* is
 * laser_transform_; range_max is the node's range_max_ (NaN and longer ranges are
 * dropped, :413,436); inverted is laser_inverted_ (descending visiting order,
 * index 0 never visited, :410). */
typedef struct ndt2d_laser_scan
{
  float angle_min, angle_increment;
  double range_max;
  int inverted;
  double laser_x, laser_y, laser_theta;
  double motion_x, motion_y, motion_theta;
} ndt2d_laser_scan;
/* d_ranges: device float[n_ranges]; d_points_xy_out: device double[n_ranges][2],
 * filled with the kept points in the reference's order; d_info_out: device
 * double[2] = {number of points kept, upper bound of max |point|}.  Asynchronous. */
int ndt2d_convert_scan_launch(ndt2d_handle h, const float * d_ranges, size_t n_ranges,
                              const ndt2d_laser_scan * scan, double * d_points_xy_out,
                              double * d_info_out);
/* Host-pointer convenience: H2D ranges, convert, D2H points (capacity n_ranges). */
int ndt2d_convert_scan(ndt2d_handle h, const float * h_ranges, size_t n_ranges,
                       const ndt2d_laser_scan * scan, double * h_points_xy_out,
                       size_t * n_points_out);
/* Conversion fused with matchScan's beam subsampling (src/scan_matcher_ndt.cpp:
 * 95-96,110): the ranges go H2D (4 B/beam), the points and the beams of
 * ndt2d_set_beams stay on the device.  Blocks for a 24-byte D2H of the counts.
 * *n_beams_out == 0 (no point kept) leaves the context without beams. */
int ndt2d_set_beams_from_ranges(ndt2d_handle h, const float * h_ranges, size_t n_ranges,
                                const ndt2d_laser_scan * scan, size_t laser_max_beams,
                                size_t * n_points_out, size_t * n_beams_out);
/* The points of the last ndt2d_set_beams_from_ranges (device pointer, valid until
 * the next conversion on this context) and their number. */
const double * ndt2d_scan_points(ndt2d_handle h, size_t * n_points_out);

/* ---- OccupancyGrid rendering on the device ----
 *
 * OccupancyGrid::getMsg (src/occupancy_grid.cpp:47-152) with its updateBounds
 * (:154-185): every beam of every scan is ray-traced from its scan pose through
 * the reference's simplified Bresenham line, cells are counted as hit / empty and
 * published as -1 (unknown) / 0 (free) / 100 (occupied, hit ratio > occ_thresh).
 * Scans are given as for ndt2d_build_grid.
 *
 * bounds_inout = {min_x_, max_x_, min_y_, max_y_} of the generator (all 0 when it
 * is new, :37-40) and n_scans_bounded = its num_scans_: as in the reference the
 * bounds are extended by the scans [n_scans_bounded, n_scans) only, and only when
 * the two counts differ (:51-54), then rounded to the resolution (:181-184).
 * info_out receives the message's meta data (:60-65).  With data_out == NULL the
 * call stops there (use it to size the buffer); otherwise data_out[width*height]
 * (row-major, y * width + x) receives the map.  A ray cell outside the grid is
 * skipped (the reference would write out of bounds: its bounds cover the scans'
 * points, not their poses).  Counts are integers, so the result is bit-identical
 * to the sequential loop. */
typedef struct ndt2d_occupancy_info
{
  double resolution;
  uint32_t width, height;
  double origin_x, origin_y;
} ndt2d_occupancy_info;
int ndt2d_occupancy_grid(ndt2d_handle h, double resolution, double occ_thresh,
                         const double * poses_xyt, const double * points_xy,
                         const size_t * offsets, size_t n_scans, size_t n_scans_bounded,
                         double * bounds_inout, ndt2d_occupancy_info * info_out,
                         signed char * data_out, size_t data_capacity);

/* ---- OccupancyGrid with resident scans and counts ----
 *
 * The same generator for a caller that publishes after every scan: the scans'
 * points, the hit / empty counters and the int8 map stay on the device, so a
 * publish after one more scan uploads that scan and its pose, traces its beams
 * into the counters of the last publish and returns the cells that can have
 * changed.  Counts are integers: the map is bit-identical to a full re-trace and
 * to ndt2d_occupancy_grid.  An ndt2d_occupancy_map is an object of its own beside
 * the context, one per generator: it holds min_x_ / max_x_ / min_y_ / max_y_ and
 * num_scans_ (:37-43), works on the context's current stream (ndt2d_set_stream)
 * and must be destroyed before ndt2d_destroy(h).  A scan's points never change
 * once appended; a caller that drops or replaces scans calls ndt2d_occmap_reset.
 *
 * The rule of ndt2d_occmap_update(map, poses_xyt, n_scans, &result), which renders
 * the first n_scans appended scans at the given poses:
 *
 * 1. n_scans below the count of the last update, or above the appended count, is
 *    NDT2D_ERR_INVALID.  A caller that drops scans calls ndt2d_occmap_reset.
 * 2. When n_scans differs from num_scans_, the bounds are extended by the scans
 *    [num_scans_, n_scans) and re-rounded, with the host arithmetic of
 *    ndt2d_occupancy_grid -- including the reference's quirk of re-rounding on
 *    every change of count (:51-54,181-184).
 * 3. Geometry comes from the bounds (:57-64).  Degenerate extents are refused as
 *    ndt2d_occupancy_grid refuses them (the object keeps the state it had).
 * 4. The mode depends on three conditions, all compared bit for bit: the counters
 *    are valid, the geometry (origin_x, origin_y, width, height) equals the last
 *    update's, and the poses of the scans already rendered equal the last
 *    update's (-0.0 against 0.0 counts as changed).
 *      all three hold and n_scans grew:          NDT2D_OCCMAP_INCREMENTAL, only the
 *                                                new scans are traced and added;
 *      all three hold and n_scans did not grow:  NDT2D_OCCMAP_UNCHANGED, nothing is
 *                                                traced, the rectangle is empty;
 *      any of the three fails:                   NDT2D_OCCMAP_FULL, the counters are
 *                                                cleared and all scans re-traced from
 *                                                the resident points (nothing but
 *                                                poses is uploaded).
 * 5. Whether a shifted origin reproduces the same cells is a question of rounding
 *    in (p - origin) / resolution, and the rule does not try to answer it: any
 *    geometry change means FULL.  That is what keeps the result exact.
 * 6. FULL finalizes the whole map, INCREMENTAL the dirty rectangle only.
 * 7. The dirty rectangle is the cell bounding box of the new scans' start and end
 *    cells, clipped to the map (Bresenham never leaves that box; cell coordinates
 *    are monotone in the map-frame coordinate, so it comes from the bounds
 *    reduction of step 2 and the new poses, without a second read-back).  FULL
 *    reports the whole map. */
typedef struct ndt2d_occupancy_map ndt2d_occupancy_map;
#define NDT2D_OCCMAP_FULL 0
#define NDT2D_OCCMAP_INCREMENTAL 1
#define NDT2D_OCCMAP_UNCHANGED 2
typedef struct ndt2d_occmap_result
{
  ndt2d_occupancy_info info;
  int mode;                  /* NDT2D_OCCMAP_* */
  uint64_t beams_traced;     /* rays walked by this update */
  uint32_t rect_x0, rect_y0, rect_w, rect_h;   /* cells that can differ from the last update */
} ndt2d_occmap_result;
/* resolution > 0 (NDT2D_ERR_INVALID otherwise). */
int ndt2d_occmap_create(ndt2d_handle h, double resolution, double occ_thresh,
                        ndt2d_occupancy_map ** out);
int ndt2d_occmap_destroy(ndt2d_occupancy_map * map);
const char * ndt2d_occmap_last_error(ndt2d_occupancy_map * map);
/* points_xy[n_points][2] in the scan's own frame (HOST; uploaded once, here);
 * n_points == 0 is allowed.  *scan_id_out (optional) = 0, 1, 2, ... */
int ndt2d_occmap_append_scan(ndt2d_occupancy_map * map, const double * points_xy,
                             size_t n_points, size_t * scan_id_out);
int ndt2d_occmap_scan_count(ndt2d_occupancy_map * map, size_t * n_out);
/* Forget scans, counters and bounds: a new generator (device memory is kept). */
int ndt2d_occmap_reset(ndt2d_occupancy_map * map);
/* poses_xyt[n_scans][3] (HOST).  See the rule above.  Returns when the bounds are
 * known; the trace may still be running (ndt2d_occmap_read waits for it). */
int ndt2d_occmap_update(ndt2d_occupancy_map * map, const double * poses_xyt, size_t n_scans,
                        ndt2d_occmap_result * result);
/* The rectangle [x0, x0 + w) x [y0, y0 + h) of the device map of the last update
 * into HOST out[h][out_row_stride] (out_row_stride >= w).  A rectangle that leaves
 * the map is NDT2D_ERR_INVALID; before the first update NDT2D_ERR_STATE. */
int ndt2d_occmap_read(ndt2d_occupancy_map * map, uint32_t x0, uint32_t y0, uint32_t w,
                      uint32_t h, signed char * out, size_t out_row_stride);
/* bounds4_out = {min_x_, max_x_, min_y_, max_y_}, *num_scans_out = num_scans_. */
int ndt2d_occmap_bounds(ndt2d_occupancy_map * map, double * bounds4_out, size_t * num_scans_out);
/* Read-only: *d_map = the DEVICE row-major map of the last update and *info its geometry, once
 * that update's trace is complete (the call waits for it).  The pointer is the object's own:
 * valid until the next ndt2d_occmap_update, _reset or _destroy, never written through.  Before
 * the first update NDT2D_ERR_STATE. */
int ndt2d_occmap_device_map(ndt2d_occupancy_map * map, const signed char ** d_map,
                            ndt2d_occupancy_info * info);

/* ---- Global localisation: particles seeded over the map's free space ----
 *
 * The first step of a filter that does not know where it is (particles uniform over the free
 * cells of an occupancy map, heading uniform) and the recovery step of augmented MCL (a share of
 * a set replaced by fresh such particles).  An ndt2d_seeder is an object of its own beside the
 * context: it owns the free table and a pinned word, launches on the context's current stream
 * (ndt2d_set_stream) and must be destroyed before ndt2d_destroy(h).  Nothing here reads or writes
 * weights, and nothing is a policy: when to inject, and how much, is the caller's.
 *
 * The free table.  A cell is free when its byte is exactly 0 (-1 unknown, 100 occupied and any
 * stray value are not).  free_cells[F] holds the row-major indices y * width + x of the free
 * cells of region4 = {x0, y0, w, h} (in cells; NULL = the whole map) in ascending order, as
 * uint32, F = ndt2d_seed_free_count.  ndt2d_seed_set_map takes a HOST map as ndt2d_occmap_read
 * gives it, ndt2d_seed_set_map_device a DEVICE one (ndt2d_occmap_device_map: nothing is
 * uploaded); both return when the table is complete, so the map may change afterwards, and both
 * replace the table of an earlier call.  Refused before anything runs, NDT2D_ERR_INVALID with a
 * message naming the item, the seeder left as it was: a NULL seeder or map; width * height zero
 * or >= 2^31; a resolution that is not finite and positive; an origin that is not finite; a
 * region that leaves the map.  F == 0 is not an error here.
 *
 * A sample is a function of (seed, step, global particle index, table, geometry) and nothing
 * else, so shards of a set draw what the whole set would (first_index, as in the noise calls).
 * Particle i takes two Philox4x32-10 blocks with key = seed (the convention of
 * ndt2d_pf_noise_launch): A = counter (first_index + i, step), B = counter (first_index + i,
 * step + 1); a call consumes TWO steps.  With a0..a3 and b0..b3 their words:
 *   u     = ((a0 >> 5) * 2^26 + (a1 >> 6)) * 2^-53          in [0, 1), the resampler's uniform
 *   k     = min(F - 1, (uint64) (u * F))                    one double multiply, truncation
 *   cell  = free_cells[k],  cx = cell mod width,  cy = cell / width
 *   ux    = ((a2 >> 8) + 0.5) * 2^-24,  uy likewise from a3   exact, in (0, 1)
 *   x     = origin_x + ((double) cx + ux) * resolution      add, multiply, add: three roundings,
 *   y     = origin_y + ((double) cy + uy) * resolution      never contracted to a fused multiply-add
 *   theta = -pi + (2 pi) * ((b0 >> 8) + 0.5) * 2^-24        pi the double M_PI, 2 pi = 2.0 * pi; one
 *                                                           multiply, one add: in (-pi, pi)
 *   v     = ((b1 >> 5) * 2^26 + (b2 >> 6)) * 2^-53          the inject draw
 * ndt2d_seed_launch writes d_poses_xyt[n][3] (DEVICE), asynchronously.  ndt2d_seed_inject_launch
 * writes particle i's sample exactly where v < probability and leaves every other particle's
 * bits alone: probability in [0, 1] (anything else, NaN included, NDT2D_ERR_INVALID); 0 writes
 * nothing; at 1 the poses are bit for bit ndt2d_seed_launch's.  *d_count (DEVICE, or NULL)
 * receives the number replaced, reduced without atomics.  Both calls: n == 0 is NDT2D_OK;
 * without a table NDT2D_ERR_STATE; with F == 0 NDT2D_ERR_STATE ("no free cell").
 *
 * ndt2d_seed_read_table copies the table to HOST out[capacity] (for tests and tools);
 * *n_out = F also when out is too small (NDT2D_ERR_INVALID then).  ndt2d_seed_set_timing /
 * _last_ms: HIP events round the three launches of the last set_map and round the last sample
 * or inject launch (0 for the one that has not been timed; neither: NDT2D_ERR_STATE). */
typedef struct ndt2d_seeder ndt2d_seeder;
int ndt2d_seed_create(ndt2d_handle h, ndt2d_seeder ** out);
int ndt2d_seed_destroy(ndt2d_seeder * seeder);
const char * ndt2d_seed_last_error(ndt2d_seeder * seeder);
int ndt2d_seed_set_map(ndt2d_seeder * seeder, const signed char * map, uint32_t width,
                       uint32_t height, double origin_x, double origin_y, double resolution,
                       const uint32_t * region4);
int ndt2d_seed_set_map_device(ndt2d_seeder * seeder, const signed char * d_map, uint32_t width,
                              uint32_t height, double origin_x, double origin_y,
                              double resolution, const uint32_t * region4);
int ndt2d_seed_free_count(ndt2d_seeder * seeder, size_t * n_out);
int ndt2d_seed_read_table(ndt2d_seeder * seeder, uint32_t * out, size_t capacity, size_t * n_out);
int ndt2d_seed_launch(ndt2d_seeder * seeder, double * d_poses_xyt, size_t n, uint64_t seed,
                      uint64_t step, uint64_t first_index);
int ndt2d_seed_inject_launch(ndt2d_seeder * seeder, double * d_poses_xyt, size_t n,
                             double probability, uint64_t seed, uint64_t step,
                             uint64_t first_index, uint64_t * d_count);
int ndt2d_seed_set_timing(ndt2d_seeder * seeder, int enabled);
int ndt2d_seed_last_ms(ndt2d_seeder * seeder, float * table_ms, float * sample_ms);

/* ---- Clearance map: the exact distance of every cell to the nearest wall ----
 *
 * A robot's centre cannot be nearer to a wall than the robot's radius, so a seeder that keeps off
 * walls, and a planner that wants an inflated map, both need the distance from every cell to the
 * nearest obstacle.  An ndt2d_clearance is an object of its own beside the context, like the
 * seeder: it launches on the context's current stream and must be destroyed before ndt2d_destroy(h).
 *
 * The quantity.  For an int8 map [height][width] a cell is an OBSTACLE when its byte is neither 0
 * nor -1 (100 and every stray value); with unknown_is_obstacle != 0, when its byte is not 0.
 * d2[y][x] (uint32) is the exact squared Euclidean distance in cells, centre to centre, to the
 * nearest obstacle cell; an obstacle cell has d2 = 0.  Outside the map there is nothing: the border
 * is no obstacle.  A map without any obstacle has NDT2D_CLEARANCE_FAR everywhere.  With a cap
 * max_cells = R > 0 every cell whose exact d2 > R * R is reported as NDT2D_CLEARANCE_FAR and every
 * other cell is exact; R = 0 is no cap.  width and height are at most 32,768 each, so d2 <=
 * 2 * 32767^2 < 2^31.  Integer arithmetic throughout, no atomics: two calls give the same bits.
 *
 * Metres enter in one place, on the host: ndt2d_clearance_min_d2 gives *min_d2 = ceil(q * q) with
 * q = clearance_m / resolution, one double divide (0.25 / 0.05 -> 25, 0.3 / 0.05 -> 36,
 * 0.3 / 0.1 -> 9).  NDT2D_ERR_INVALID: a clearance that is negative or not finite, a resolution
 * that is not finite and positive, a negative max_cells, a min_d2 above 2^31, or a cap R > 0 with
 * min_d2 > R * R (the capped transform could not tell such cells apart).  A cell HAS THE CLEARANCE
 * exactly when d2 >= min_d2, so NDT2D_CLEARANCE_FAR always has it.  A caller who wants an integer
 * radius r passes min_d2 = r * r itself.
 *
 * ndt2d_clearance_compute takes a HOST map, ndt2d_clearance_compute_device a DEVICE one
 * (ndt2d_occmap_device_map: nothing is uploaded).  The transform always covers the whole map.
 * ndt2d_clearance_mask makes the object's own copy of that map in which every free cell (byte 0)
 * with d2 < min_d2 is byte 99 (the "inscribed" value of the nav2 costmap convention) and every
 * other byte is unchanged: given to ndt2d_seed_set_map_device, whose rule "byte exactly 0" drops
 * the 99s, it seeds only cells that have the clearance.  compute* and mask return when complete,
 * so the source map may change afterwards.  *d_d2 (ndt2d_clearance_device) and *d_masked_map are
 * the object's own, read-only, valid until the next compute*, mask or destroy.
 * ndt2d_clearance_read / _read_mask copy a rectangle to HOST out[h][out_row_stride] (in elements,
 * >= w), as ndt2d_occmap_read does.
 *
 * Refused before anything is allocated or launched, NDT2D_ERR_INVALID with a message naming the
 * item, the object (and its earlier result) left as it was: NULL arguments, a zero width or
 * height, a side above 32,768, a negative max_cells, a rectangle that leaves the map.  read,
 * device and mask before the first compute, and read_mask before a mask of the last compute, are
 * NDT2D_ERR_STATE.  ndt2d_clearance_set_timing / _last_ms: HIP events round the four launches of
 * the last compute and round the last mask launch (0 for the one not timed; neither:
 * NDT2D_ERR_STATE). */
#define NDT2D_CLEARANCE_FAR 0xFFFFFFFFu
typedef struct ndt2d_clearance ndt2d_clearance;
int ndt2d_clearance_create(ndt2d_handle h, ndt2d_clearance ** out);
int ndt2d_clearance_destroy(ndt2d_clearance * clearance);
const char * ndt2d_clearance_last_error(ndt2d_clearance * clearance);
int ndt2d_clearance_compute(ndt2d_clearance * clearance, const signed char * map, uint32_t width,
                            uint32_t height, int unknown_is_obstacle, int64_t max_cells);
int ndt2d_clearance_compute_device(ndt2d_clearance * clearance, const signed char * d_map,
                                   uint32_t width, uint32_t height, int unknown_is_obstacle,
                                   int64_t max_cells);
int ndt2d_clearance_min_d2(double clearance_m, double resolution, int64_t max_cells,
                           uint32_t * min_d2);
int ndt2d_clearance_read(ndt2d_clearance * clearance, uint32_t x0, uint32_t y0, uint32_t w,
                         uint32_t h, uint32_t * out, size_t out_row_stride);
int ndt2d_clearance_device(ndt2d_clearance * clearance, const uint32_t ** d_d2, uint32_t * width,
                           uint32_t * height);
int ndt2d_clearance_mask(ndt2d_clearance * clearance, uint32_t min_d2,
                         const signed char ** d_masked_map);
int ndt2d_clearance_read_mask(ndt2d_clearance * clearance, uint32_t x0, uint32_t y0, uint32_t w,
                              uint32_t h, signed char * out, size_t out_row_stride);
int ndt2d_clearance_set_timing(ndt2d_clearance * clearance, int enabled);
int ndt2d_clearance_last_ms(ndt2d_clearance * clearance, float * transform_ms, float * mask_ms);

/* ---- Pose clusters: the pose of the heaviest cluster of a particle set ----
 *
 * While a globally seeded set settles, its belief has several modes; the mean over all particles
 * lies in none of them.  An ndt2d_clusterer groups the particles d_poses_xyt[n][3] with weights
 * d_weights[n] (both DEVICE; d_weights NULL = every weight 1.0 / (double) n) into connected
 * clusters of occupied pose bins and returns the max_clusters heaviest with updateStatistics'
 * quantities of each.  The particles never leave the device; one small block is read back.  It is
 * an object of its own beside the context (as the seeder and the resampler): it launches on the
 * context's current stream and must be destroyed before ndt2d_destroy(h).  Nothing calls it by
 * default and nothing here is a policy: what share makes a filter "localised" is the caller's.
 * (ndt_2d_amd/csrc/cluster/ndt2d_cluster_fn.h holds this arithmetic as plain C++.)
 *
 * Bins.  kx = floor(x / cell_x), ky = floor(y / cell_y): floor, not the KLD tree's truncation,
 * which makes the bin at 0 twice as wide.  ktheta = min(n_theta - 1, (int) ((t + pi) / (2 pi) *
 * n_theta)) with t = theta normalised into [-pi, pi): r = fmod(theta, 2 pi); r += 2 pi where
 * r < -pi; then r -= 2 pi where r >= pi (pi the double M_PI, 2 pi = 2.0 * pi; the add, the
 * quotient and the product each rounded on their own).  Defaults cell_x = cell_y = 0.5,
 * n_theta = 24; ndt2d_cluster_set_bins changes them (cells finite and positive, n_theta >= 1).
 *
 * Left out.  A particle is left out, counted in n_left_out and labelled 0xFFFFFFFF when its pose is
 * not finite, when |x / cell_x| or |y / cell_y| is 2^30 or more, or when its weight is not in
 * [0, 1] (a NaN is not).
 *
 * Adjacency.  Two occupied bins are neighbours when their keys differ by at most 1 in each
 * coordinate, ktheta taken modulo n_theta (the 26-neighbourhood; a blob at heading +-pi is one
 * cluster; with n_theta of 1 or 2 a bin is its own or its twin's heading neighbour).  A cluster is
 * a connected component; its LABEL is the smallest particle index in it.
 *
 * Mass.  q_i = (uint64) (w_i * 2^40), Q = sum q_i: integer adds, the same Q in any order.  Clusters
 * are ranked by (Q descending, label ascending).  A weight below 2^-40 has q = 0 and does not count
 * towards the rank; it does count towards W and the statistics.  No floating-point atomic is used
 * anywhere.  (max_particles <= 2^23 keeps Q below 2^63 for any weights in [0, 1].)
 *
 * Statistics of each of the first max_clusters clusters of that order (1 .. 16, default 8),
 * restricted to the cluster and renormalised by its own W = sum w_i: the means of x and y, the
 * circular mean atan2(sum w sin theta, sum w cos theta), the CENTRED second moments
 * sum w (x - mean_x)(y - mean_y) / W for xx, xy and yy, sum w d^2 / W with d = theta_i - mean_theta
 * normalised as above, and the particle count.  Every double sum is a fixed tree over fixed chunks
 * of the index order: two calls on the same input give the same bits.  (A cluster whose weights are
 * all 0 has W = 0 and statistics that are not numbers; it ranks behind every cluster with mass.)
 *
 * ndt2d_cluster_launch is asynchronous: it queues the keys, the bin table, the bin list, the
 * neighbour table and the first label rounds, and keeps the two pointers until the fetch, which
 * reads them again.  ndt2d_cluster_fetch waits, queues further label rounds while the last one
 * still lowered a label (more than B + 2 rounds: NDT2D_ERR_INTERNAL), then the masses, the
 * selection and the statistics, and copies the header and *n_records = min(max_clusters, C) records,
 * heaviest first, to HOST records_out[capacity] (capacity below that: NDT2D_ERR_INVALID, *n_records
 * still set).  A second fetch returns the same block.  n == 0 is legal and gives zeros.  Refused
 * before anything is allocated or queued, NDT2D_ERR_INVALID with a message, the object left as it
 * was: a cell that is not finite and positive, n_theta < 1, max_clusters outside 1 .. 16,
 * n > max_particles, NULL poses with n > 0.  ndt2d_cluster_read_labels copies every particle's
 * label of the last fetched call to HOST out[n] (for tests and tools).  ndt2d_cluster_set_timing /
 * _last_ms: HIP events round five phases of the last fetched call, in ms: {keys and table, bin
 * list and neighbours, label rounds (with the host's reads between them), masses and selection,
 * statistics and read-back}. */
#define NDT2D_CLUSTER_MAX_RECORDS 16
typedef struct ndt2d_cluster_header
{
  uint64_t n;            /* particles of the call */
  uint64_t n_left_out;
  uint64_t n_bins;       /* B: occupied bins */
  uint64_t n_clusters;   /* C: all of them, also beyond max_clusters */
  uint64_t rounds;       /* label rounds run, the one that changed nothing included */
  double w_total;        /* sum of the weights of the particles that are not left out */
} ndt2d_cluster_header;
typedef struct ndt2d_cluster_record
{
  uint32_t label;        /* the smallest particle index of the cluster */
  uint32_t count;        /* its particles */
  double mass;           /* Q * 2^-40 */
  double weight;         /* W */
  double mean_x, mean_y, mean_theta;
  double cxx, cxy, cyy, var_theta;
} ndt2d_cluster_record;
typedef struct ndt2d_clusterer ndt2d_clusterer;
int ndt2d_cluster_create(ndt2d_handle h, size_t max_particles, ndt2d_clusterer ** out);
int ndt2d_cluster_destroy(ndt2d_clusterer * clusterer);
const char * ndt2d_cluster_last_error(ndt2d_clusterer * clusterer);
int ndt2d_cluster_set_bins(ndt2d_clusterer * clusterer, double cell_x, double cell_y, int n_theta);
int ndt2d_cluster_set_max_clusters(ndt2d_clusterer * clusterer, int max_clusters);
int ndt2d_cluster_launch(ndt2d_clusterer * clusterer, const double * d_poses_xyt,
                         const double * d_weights, size_t n);
int ndt2d_cluster_fetch(ndt2d_clusterer * clusterer, ndt2d_cluster_header * header_out,
                        ndt2d_cluster_record * records_out, size_t capacity, size_t * n_records);
int ndt2d_cluster_read_labels(ndt2d_clusterer * clusterer, uint32_t * out, size_t n);
int ndt2d_cluster_set_timing(ndt2d_clusterer * clusterer, int enabled);
int ndt2d_cluster_last_ms(ndt2d_clusterer * clusterer, float * ms5);

/* ---- device memory for hosts without a GPU runtime of their own ----
 *
 * The *_launch entry points take device pointers.  A host that already manages
 * device memory (PyTorch, a HIP application) passes its own; the C++ mirrors in
 * ndt_2d_amd/plugin/ (particle_filter_hip.hpp) use these four.  Copies are
 * ordered on the context's stream and return when the data has arrived. */
int ndt2d_device_alloc(ndt2d_handle h, size_t bytes, void ** d_out);
int ndt2d_device_free(ndt2d_handle h, void * d_ptr);
int ndt2d_copy_to_device(ndt2d_handle h, void * d_dst, const void * h_src, size_t bytes);
int ndt2d_copy_to_host(ndt2d_handle h, void * h_dst, const void * d_src, size_t bytes);
/* The same copies queued on the context's stream without the wait: the host buffer must stay
 * valid (and, for a copy that really is asynchronous, be pinned: ndt2d_host_alloc) until
 * ndt2d_synchronize.  A multi-device matcher feeds its devices with these. */
int ndt2d_copy_to_device_async(ndt2d_handle h, void * d_dst, const void * h_src, size_t bytes);
int ndt2d_copy_to_host_async(ndt2d_handle h, void * h_dst, const void * d_src, size_t bytes);

/* Pinned, GPU-mapped host memory: poses / weights buffers allocated here are read and
 * written by the kernels of the host-pointer entry points directly over PCIe (no staging
 * copy, no copy command); the C++ ParticleFilter mirror keeps its particles in it. */
int ndt2d_host_alloc(ndt2d_handle h, size_t bytes, void ** out);
/* h may be NULL once the context that allocated `ptr` has been destroyed (nothing of its
 * stream can then be in flight): the buffer outlives its context if the caller wants so. */
int ndt2d_host_free(ndt2d_handle h, void * ptr);

/* HIP events around the dominant kernel of every launch (ndt2d_last_launch_ms /
 * ndt2d_launch_history_ms) are recorded by default; a latency-critical host (the
 * pluginlib shim) turns them off: a recorded event holds the stream up for ~5.5 us where
 * consecutive kernels otherwise start back to back, and the pair costs ~4.5 us of host
 * time per call. */
int ndt2d_set_timing(ndt2d_handle h, int enabled);

/* Block until everything launched on the context's stream has finished. */
int ndt2d_synchronize(ndt2d_handle h);
/* GPU time (HIP events on the launch stream) of the dominant kernel -- the
 * search / scoring kernel, without the few-microsecond final reduction -- of the
 * most recent ndt2d_match_launch / ndt2d_score_poses_launch.  Synchronises.
 * *n_kernels (optional) = kernels launched by that call. */
int ndt2d_last_launch_ms(ndt2d_handle h, float * ms, int * n_kernels);
/* The same figure for the last launches, oldest first (the context keeps the
 * event pairs of its last NDT2D_TIMING_HISTORY launches): lets a caller queue
 * launches back to back and read the kernel durations afterwards.  Writes at
 * most `capacity` values, *n_out = how many; blocks until the newest finished. */
#define NDT2D_TIMING_HISTORY 256
int ndt2d_launch_history_ms(ndt2d_handle h, float * ms_out, size_t capacity, size_t * n_out);
/* Tuning / introspection: name of the kernel variant the last launch used. */
const char * ndt2d_last_variant(ndt2d_handle h);
/* "auto" (the default) picks the candidate mapping of the match search by the size
 * of the lattice: lane-per-candidate with the beams split across the waves of a block
 * ("small") below 4,096 (theta, 8x8 patch) work items -- the plugin's default search is
 * 720 -- and lane-per-candidate with persistent waves ("lane") above; wave-per-candidate
 * ("wave") where neither applies (search windows beyond 1,024 cells, NaN beams).  All give
 * the oracle's result; they differ from each other in the last bits of a score
 * (summation order).
 * Force a kernel variant (testing / A-B measurement): "auto", "lds", "global"
 * (grid placement), "wave", "wave-lds", "wave-global", "lane", "small" (candidate mapping
 * of the match search), "lane-noskip" / "small-noskip" (the lane mappings with every term
 * evaluated: the bit-exactness controls of their skipping), "batched" (pose batches of
 * at most 2,048 on the batched particle kernel instead of block-per-pose), "dense" (particle
 * scoring without compaction), "compact-exact" (particle scoring with the exact
 * FP64 phase A: the bit-exactness control of the FP32 screen). */
int ndt2d_set_variant(ndt2d_handle h, const char * name);
/* A batch of 131,072 poses or more handed over in ordinary host memory (ndt2d_score_poses,
 * ndt2d_pf_measure: ParticleFilter::measure of a large filter, reference
 * src/particle_filter.cpp:78-89) is cut into pieces: piece k + 1 is uploaded on a stream of its own
 * while piece k is scored, raw scores travel back under the piece after.  The raw scores do not
 * depend on the cut (bit-identical), the pieces' moment sums are added in piece order.
 * CONTRACT on the statistics: the eight moment sums (total weight, sum w x, ...) are sums of a
 * million terms whose ORDER follows the cut -- pieces here, devices in a multi-device matcher
 * (ndt2d_matcher_set_multi_thresholds), blocks of the one-launch form -- so the normalised weights,
 * mean and covariance of ndt2d_pf_measure / ndt2d_score_poses(h_stats) agree between any two
 * settings of this knob (and between one and several devices) to within 64 ulps of the sums'
 * magnitude, not bit for bit; a caller that needs the same bits every time fixes the knob.
 * tests/test_gpu_pose_batch_pipeline.py holds every setting to that bound.
 * pieces: 0 = default (4), 1 = off (one upload, one launch, one download), at most 16. */
int ndt2d_set_pipeline_pieces(ndt2d_handle h, int pieces);
/* Pieces the last ndt2d_score_poses / ndt2d_pf_measure was cut into (1: not pipelined). */
int ndt2d_last_pipeline_pieces(ndt2d_handle h);

/* ------------------------------------------------------------------------ */
/* (2) matcher layer: ndt_2d::ScanMatcherNDT restated over the device layer  */
/* ------------------------------------------------------------------------ */

typedef struct ndt2d_matcher ndt2d_matcher;

int ndt2d_matcher_create(ndt2d_matcher ** out, int device_id);
/* One matcher over n_dev GPUs of this process (`ndt2d_create(handle*, const int*
 * device_ids, int n_dev)`): the plugin object the unchanged node holds, with the 8-GPU split of
 * the loop-closure search (reference src/ndt_mapper.cpp:634-643 calls a plain matchScan) behind
 * it.  One device context and stream per entry of device_ids, all driven by the calling thread;
 * grid, beams and search tables are replicated by host-to-device copies.
 *
 *   matchScan   theta steps dealt round-robin (device r takes r, r + n_dev, ...: the cost of a
 *               step varies across the angular range), one 12-double record per device, the
 *               records exchanged ONCE and combined with the reference's first-wins rule
 *               (strict `<` in visiting order, src/scan_matcher_ndt.cpp:128: the lower score,
 *               between equal scores the lower flat index), accumulators summed in device order;
 *   scorePoses / pf_measure   contiguous particle ranges, one exchange of the [n_dev, 8] moment
 *               sums (the "total particle weight" of src/particle_filter.cpp:166-174), and the
 *               theta variance of the reference's second pass (:213-217) with a second one.
 *
 * The exchange (ndt2d_matcher_set_exchange): "rccl" = ONE in-place ncclAllReduce(sum) of the
 * [n_dev, 12] (or [n_dev, 8]) table per device -- every device fills its own row, x + 0 is
 * exact -- in one ncclGroupStart / ncclGroupEnd over single-process communicators
 * (ncclCommInitAll; xGMI between the devices), the table then read back from the first device;
 * "host" = no collective: every device's final reduction writes its record into its context's
 * host-coherent result block and the host combines them (a device may then appear more than
 * once in device_ids: several contexts on one GPU, which RCCL refuses).  "auto" (default):
 * "rccl" when all devices differ and librccl.so.1 loads, "host" otherwise.  Both give the same
 * bits.
 *
 * Dealing: one persistent worker thread per device beyond the first (made here, parked on a
 * condition variable after ~200 us without work), the calling thread drives the first device:
 * all devices' uploads and launches go out side by side (ndt2d_matcher_last_fanout_us: when
 * each device's launch had been queued, from the call's start).  Sharded particle sets run
 * their whole share on the device's thread -- upload, scoring, the sums' meeting on the host
 * (a barrier between the threads, no stream synchronisation), updateStatistics with the totals
 * as kernel arguments, the weights' way back.
 *
 * Work smaller than the thresholds of ndt2d_matcher_set_multi_thresholds (candidates x beams
 * of a search, default 1e9 -- ~0.3 ms of one GPU; particles x beams of a batch, default 2e8
 * -- ~0.2 ms: BASELINE configs[4], 7.2e8, is sharded) and every single-pose call stay on the
 * first device.  ndt2d_matcher_set_multi_min_units sets both to one value.
 * n_dev == 1 behaves exactly as ndt2d_matcher_create. */
int ndt2d_matcher_create_multi(ndt2d_matcher ** out, const int * device_ids, int n_dev);
int ndt2d_matcher_destroy(ndt2d_matcher * m);
const char * ndt2d_matcher_last_error(ndt2d_matcher * m);
int ndt2d_matcher_device_count(ndt2d_matcher * m);
/* The device context of rank `rank` (0 <= rank < device_count), NULL otherwise. */
ndt2d_handle ndt2d_matcher_device_at(ndt2d_matcher * m, int rank);
int ndt2d_matcher_set_exchange(ndt2d_matcher * m, const char * mode);
int ndt2d_matcher_set_multi_min_units(ndt2d_matcher * m, double units);
int ndt2d_matcher_set_multi_thresholds(ndt2d_matcher * m, double min_search_units, double min_pose_units);
int ndt2d_matcher_get_multi_thresholds(ndt2d_matcher * m, double * min_search_units, double * min_pose_units);
/* Of the last call that was dealt to the devices: for device r, microseconds from the call's
 * start until its (first) launch had been queued -- out_us[r], r < min(capacity, n_dev);
 * *n_out = n_dev (0 if no call was dealt yet). */
int ndt2d_matcher_last_fanout_us(ndt2d_matcher * m, double * out_us, size_t capacity, size_t * n_out);
/* What the last matchScan / scorePoses / pf_measure ran as: the kernel variant of the first
 * device (ndt2d_last_variant), prefixed "multi[n]/rccl/" or "multi[n]/host/" when the call was
 * dealt to n devices. */
const char * ndt2d_matcher_last_variant(ndt2d_matcher * m);
/* ndt2d_set_timing on every device of the matcher. */
int ndt2d_matcher_set_timing(ndt2d_matcher * m, int enabled);
/* The (first) device context the matcher drives (for sharded launches / streams).  The matcher
 * remembers which beams it put there (a scan that arrives again is not uploaded again):
 * it must remain the only writer of this context's beams. */
ndt2d_handle ndt2d_matcher_device(ndt2d_matcher * m);

/* ScanMatcherNDT::initialize (src/scan_matcher_ndt.cpp:35-47): the six
 * declared parameters (defaults 0.25, 0.0025, 0.1, 0.005, 0.05, 100) and
 * range_max. */
int ndt2d_matcher_initialize(ndt2d_matcher * m, double ndt_resolution,
                             double search_angular_resolution, double search_angular_size,
                             double search_linear_resolution, double search_linear_size,
                             size_t laser_max_beams, double range_max);
/* ScanMatcherNDT::addScans (src/scan_matcher_ndt.cpp:49-74): scan k has pose
 * poses_xyt[3k..3k+2] and robot-frame points
 * points_xy[2*offsets[k] .. 2*offsets[k+1]).  Builds the NDT on the host with
 * the reference's incremental formulas (src/ndt_model.cpp:50-103,132-160) and
 * uploads it. */
int ndt2d_matcher_add_scans(ndt2d_matcher * m, const double * poses_xyt,
                            const double * points_xy, const size_t * offsets, size_t n_scans);
/* Where addScans builds the NDT: "host" (C++ on the host, then upload), "device"
 * (ndt2d_build_grid) or "auto" (device from 73,728 map points up: ~100 scans of 720 beams).  Both give
 * bit-identical grids.  "fused" (opt-in): ndt2d_build_grid_small when the map is within its
 * limits, otherwise exactly what "auto" does; after a fused build there is no host NDT, as
 * after a device build (scoreScan / scorePoints take the device single-pose path). */
int ndt2d_matcher_set_build_mode(ndt2d_matcher * m, const char * mode);
/* Resident scans (ndt2d_scanstore) at matcher level.  store_scan keeps a scan's points on every
 * device of the matcher and returns its id (ids count from 0); add_scans_by_id is addScans of the
 * stored scans ids[0..n_scans) in that order with the poses given -- every device builds its own
 * copy through the fused build, as add_scans replicates builds -- and gives the grid add_scans
 * gives for the same scans and poses.  A map beyond the fused build's limits, an unknown id or a
 * non-finite pose: NDT2D_ERR_INVALID, the NDT in place stays.  drop_scans forgets every stored
 * scan.  The stores hold up to 262,144 points and 4,096 scans per device. */
int ndt2d_matcher_store_scan(ndt2d_matcher * m, const double * points_xy, size_t n_points, size_t * id_out);
int ndt2d_matcher_add_scans_by_id(ndt2d_matcher * m, const double * poses_xyt, const size_t * ids,
                                  size_t n_scans);
int ndt2d_matcher_drop_scans(ndt2d_matcher * m);
/* How the NDT in place was built: "build/fused-small-map" (the fused build: mode "fused" within
 * its limits, add_scans_by_id), "build/device" (ndt2d_build_grid), "build/host", or "" without
 * an NDT. */
const char * ndt2d_matcher_last_build(ndt2d_matcher * m);
/* ndt2d_set_eigenvalue_form for the host build and every device of the matcher. */
int ndt2d_matcher_set_eigenvalue_form(ndt2d_matcher * m, const char * form);
/* ScanMatcherNDT::matchScan (src/scan_matcher_ndt.cpp:76-149).  *score_out =
 * the function's return value (best_score / scan_points_to_use; 0.0 and
 * outputs untouched when no NDT, :80).  pose_inout[3] is written only when a
 * candidate scores < 0 (:128-134); covariance_out[9] row-major (:146). */
int ndt2d_matcher_match_scan(ndt2d_matcher * m, const double * scan_pose_xyt,
                             const double * points_xy, size_t n_points, double * pose_inout,
                             double * covariance_out, double * score_out);
/* Same search, additionally returning the raw score of every candidate
 * (all_scores, host, capacity all_scores_cap), the candidate count and the
 * winner's flat index; any of the extra outputs may be NULL. */
int ndt2d_matcher_match_scan_ex(ndt2d_matcher * m, const double * scan_pose_xyt,
                                const double * points_xy, size_t n_points,
                                double * pose_inout, double * covariance_out,
                                double * score_out, double * all_scores,
                                size_t all_scores_cap, size_t * n_candidates_out,
                                uint64_t * best_index_out);
/* The loop-closure thread's inner loop in one call (ndt2d_closure_match with the matcher's own
 * parameters and stored scans, on the first device).  For candidate k of K the outputs are
 * what this sequence gives on the same matcher:
 *     ndt2d_matcher_reset; ndt2d_matcher_add_scans_by_id(poses_k, ids_k, n_k);
 *     ndt2d_matcher_match_scan_ex(scan_pose, points, ...)
 * with ids_k / poses_k = ids / poses_xyt[cand_offsets[k] .. cand_offsets[k + 1]) (flat arrays,
 * poses three doubles an entry).  Every candidate starts from the same scan_pose.
 *   poses_out[3 k ..]        written only when a lattice candidate of k scores below 0 (as
 *                            match_scan's pose_inout): the caller pre-initialises it;
 *   covariances_out[9 k ..]  row-major;  scores_out[k]  match_scan's return value;
 *   best_index_out[k]        (optional) the winner's flat index, NDT2D_NO_INDEX if none;
 *   all_scores               (optional) [K][lattice] raw scores, all_scores_cap doubles: only
 *                            filled when it holds them all;  *n_lattice_out (optional) the
 *                            lattice size n_th * n_lin * n_lin.
 * A candidate map whose record comes back marked as a near tie is settled by running the three
 * sequential calls for that candidate alone -- the existing adjudication, counted by
 * ndt2d_matcher_adjudication_stats as any other.  A search launched ahead by score_scan is
 * waited out and dropped first.  On return the matcher holds no NDT (has_ndt == 0), as after
 * the reset() every iteration of the reference's loop begins with.  Refusals are those of
 * ndt2d_closure_match (NDT2D_ERR_INVALID, the message names the candidate, nothing launched,
 * the NDT in place stays). */
int ndt2d_matcher_match_candidates(ndt2d_matcher * m, const double * scan_pose_xyt,
                                   const double * points_xy, size_t n_points,
                                   const size_t * cand_offsets, const size_t * ids,
                                   const double * poses_xyt, size_t n_candidates,
                                   double * poses_out, double * covariances_out,
                                   double * scores_out, uint64_t * best_index_out,
                                   double * all_scores, size_t all_scores_cap,
                                   size_t * n_lattice_out);
/* The batched call's closure object (made by the first match_candidates; NULL before), for
 * ndt2d_closure_set_timing / _last_ms. */
ndt2d_closure * ndt2d_matcher_closure(ndt2d_matcher * m);
/* matchScan from K start poses against the NDT in place, in one call (ndt2d_starts_match with
 * the matcher's own parameters, on the first device): relocalisation in a loaded map, several
 * hypotheses of a tracker.  For start k the outputs are what
 *     ndt2d_matcher_match_scan_ex(m, starts_xyt + 3 k, points, ...)
 * gives on the same matcher, with match_candidates' conventions: poses_out[3 k ..] is written
 * only when a lattice candidate of k scores below 0, best_index_out[k] is NDT2D_NO_INDEX without
 * a winner, all_scores [K][lattice] is only filled when it holds them all, *n_lattice_out the
 * lattice size (0 with no NDT in place: every score is then 0.0 and nothing else is written,
 * src/scan_matcher_ndt.cpp:80).  A start whose record comes back marked as a near tie is settled
 * by the sequential call for that start alone (ndt2d_matcher_adjudication_stats counts it); no
 * points or an empty lattice go through the sequential call per start.  A search launched ahead
 * by score_scan is waited out and dropped first.  The NDT stays in place.  A non-finite start:
 * NDT2D_ERR_INVALID, "start k" in the message, nothing launched. */
int ndt2d_matcher_match_starts(ndt2d_matcher * m, const double * starts_xyt, size_t n_starts,
                               const double * points_xy, size_t n_points, double * poses_out,
                               double * covariances_out, double * scores_out,
                               uint64_t * best_index_out, double * all_scores,
                               size_t all_scores_cap, size_t * n_lattice_out);
/* The batched call's object (made by the first match_starts with an NDT in place; NULL before), for
 * ndt2d_starts_set_timing / _last_ms. */
ndt2d_starts * ndt2d_matcher_starts(ndt2d_matcher * m);
/* matchScan over a lattice of the CALL's sizes -- linear_size / linear_res, angular_size /
 * angular_res, the offsets of ndt2d_search_offsets -- against the NDT in place, by the wide search
 * (ndt2d_wide_match on the first device): what replaces matchScan where the window is metres wide.
 * The scan is subsampled with the matcher's laser_max_beams as matchScan subsamples it; the
 * matcher's own lattice is not touched.  tile_steps == 0 keeps the object's tile steps.
 * pose_out[3] = the winner's (dx, dy, dtheta) correction (written only with a winner), *score_out =
 * best / N (:148), *best_index_out = its flat index in the call's lattice (NDT2D_NO_INDEX: none),
 * *near_tie_out = 1 when another candidate lies within the near-tie tolerance (marked, not
 * settled), stats_out[2] = {tile jobs scored, tile jobs in all}; all optional but score_out.  No
 * covariance: the sums need every candidate (ndt2d_matcher_refine_scans with neighbourhood 9 on
 * the winner gives one).  The bound image is kept between calls while the matcher has not built,
 * installed or dropped an NDT in between.  No NDT in place: score 0.0, nothing else written.
 * A search launched ahead by score_scan is waited out and dropped first.  NDT2D_ERR_INVALID,
 * nothing launched: a non-finite pose, sizes or resolutions ndt2d_search_offsets refuses, what
 * ndt2d_wide_match refuses (its message follows "match_wide: "). */
int ndt2d_matcher_match_wide(ndt2d_matcher * m, const double * scan_pose_xyt, const double * points_xy,
                             size_t n_points, double linear_size, double linear_res,
                             double angular_size, double angular_res, uint32_t tile_steps,
                             double * pose_out, double * score_out, uint64_t * best_index_out,
                             int * near_tie_out, uint64_t * stats_out);
/* The wide search's object (made by the first match_wide with an NDT in place; NULL before), for
 * ndt2d_wide_set_tile / _set_timing / _last_ms. */
ndt2d_wide * ndt2d_matcher_wide(ndt2d_matcher * m);
/* matchScan of K jobs -- (scan, pose) pairs -- against the NDT in place, in one call
 * (ndt2d_scans_match with the matcher's own parameters, on the first device): the localisation
 * branch (src/ndt_mapper.cpp:547-566) for a fleet on one map, a replayed bag, a graph's scans
 * after an optimisation.  Scan s is points_xy[2 * point_offsets[s] .. 2 * point_offsets[s + 1]),
 * point_offsets[n_scans + 1] non-decreasing; job_scan[k] names the scan of job k (NULL: job k
 * uses scan k, n_scans == n_jobs).  Each scan a job names is subsampled once, as matchScan
 * subsamples it.  For job k the outputs are what
 *     ndt2d_matcher_match_scan_ex(m, jobs_xyt + 3 k, the points of scan job_scan[k], ...)
 * gives on the same matcher, with match_starts' conventions: poses_out[3 k ..] is written only
 * when a lattice candidate of k scores below 0, best_index_out[k] is NDT2D_NO_INDEX without a
 * winner, all_scores [K][lattice] is only filled when it holds them all, *n_lattice_out the
 * lattice size (0 with no NDT in place: every score is then 0.0 and nothing else is written,
 * src/scan_matcher_ndt.cpp:80).  A job whose record comes back marked as a near tie is settled
 * by the sequential call for that job alone (ndt2d_matcher_adjudication_stats counts it); jobs
 * of a scan without points, or an empty lattice, go through the sequential call.  A search
 * launched ahead by score_scan is waited out and dropped first.  The NDT stays in place.
 * NDT2D_ERR_INVALID, nothing launched: a non-finite job pose or a scan index out of range
 * ("job k" in the message), point_offsets that decrease ("scan s"), job_scan == NULL with
 * n_scans != n_jobs. */
int ndt2d_matcher_match_scans(ndt2d_matcher * m, const double * jobs_xyt, const uint32_t * job_scan,
                              size_t n_jobs, const double * points_xy, const size_t * point_offsets,
                              size_t n_scans, double * poses_out, double * covariances_out,
                              double * scores_out, uint64_t * best_index_out, double * all_scores,
                              size_t all_scores_cap, size_t * n_lattice_out);
/* The batched call's object (made by the first match_scans with an NDT in place; NULL before), for
 * ndt2d_scans_set_timing / _last_ms. */
ndt2d_scans * ndt2d_matcher_scans(ndt2d_matcher * m);
/* Newton NDT registration of K jobs -- (scan, pose) pairs -- against the NDT in place, in one call
 * (ndt2d_refine_run on the first device): from each job's pose -- a lattice winner of match_scans,
 * an odometry guess -- to the optimum of the scan's score under it.  Scans, jobs and job_scan as
 * in match_scans; each scan a job names is subsampled once with the matcher's laser_max_beams, as
 * matchScan / scorePoints subsample it.  Per job k:
 *     poses_out[3 k ..]        the ABSOLUTE pose reached (not a correction)
 *     scores_out[k]            f / N at that pose: what score_points gives there
 *     start_scores_out[k]      f / N at the job's pose                       (optional)
 *     gradients_out[3 k ..]    g / N                                         (optional)
 *     hessians_out[9 k ..]     H / N, row-major 3 x 3, symmetric             (optional)
 *     status_out[k]            NDT2D_REFINE_*
 *     evals_out[2 k ..]        evaluations, accepted steps                   (optional)
 * No NDT in place: every score is 0.0, the poses are the jobs' own, status NO_OVERLAP, no
 * evaluation (src/scan_matcher_ndt.cpp:159); jobs of a scan without points get the same.  A
 * search launched ahead by score_scan is waited out and dropped first.  The NDT stays in place;
 * the beams and the prepared search of the context are not touched.  NDT2D_ERR_INVALID, nothing
 * launched: a non-finite job pose or a scan index out of range ("job k" in the message),
 * point_offsets that decrease ("scan s"), job_scan == NULL with n_scans != n_jobs, max_evals == 0,
 * a tolerance that is negative or not finite. */
int ndt2d_matcher_refine_scans(ndt2d_matcher * m, const double * jobs_xyt, const uint32_t * job_scan,
                               size_t n_jobs, const double * points_xy, const size_t * point_offsets,
                               size_t n_scans, uint32_t max_evals, double tol_lin, double tol_ang,
                               double * poses_out, double * scores_out, double * start_scores_out,
                               double * gradients_out, double * hessians_out, int32_t * status_out,
                               uint32_t * evals_out);
/* The call's object (made by the first refine_scans with an NDT in place; NULL before), for
 * ndt2d_refine_set_timing / _last_ms. */
ndt2d_refine * ndt2d_matcher_refine(ndt2d_matcher * m);
/* The neighbourhood of the later refine_scans calls: 1 (the default) or 9 cells per point
 * (ndt2d_refine_set_neighbourhood; anything else: NDT2D_ERR_INVALID, the value stays).  Kept in
 * the matcher -- the call's object is only made by the first refine_scans -- and applied to every
 * later call.  With 9, scores_out / start_scores_out are f / N of the 3 x 3 objective: no longer
 * what score_points gives at that pose; gradients_out / hessians_out are that objective's.  For a
 * covariance of a refined pose: ndt2d_refine_covariance of hessians_out's six entries times N (the
 * beams in use, min(laser_max_beams, the scan's points)). */
int ndt2d_matcher_set_refine_neighbourhood(ndt2d_matcher * m, uint32_t cells);
int ndt2d_matcher_refine_neighbourhood(ndt2d_matcher * m, uint32_t * out);
/* Match verification of K jobs -- (scan, pose) pairs -- against the NDT in place, in one call
 * (ndt2d_verify_run on the first device, as refine_scans): which beams of each scan the map
 * explains at the job's pose ("Match verification" above).  Scans, jobs and job_scan as in
 * refine_scans.  max_beams: 0 takes every point of a scan (filtering a scan before it is stored);
 * otherwise min(max_beams, the scan's points) points by the subsampling rule of matchScan /
 * scorePoints (:165-166,171) -- with the matcher's laser_max_beams the verdict is about the beams
 * the score was computed from.  Per job k:
 *     records_out[8 k ..]       {n_beams, n_off, n_unseen, n_outlier, n_inlier, n_pierced, n_walked, 0}
 *     beam_offsets_out[k]       where job k's beams start in the per-beam arrays; [K]: their total   (optional, K + 1)
 *     beam_class_out, beam_m2_out, beam_cells_out   ndt2d_verify_run's per-beam arrays          (optional)
 * beam_cap: the beams the per-beam arrays hold; fewer than the jobs' beams: NDT2D_ERR_INVALID, the
 * message says how many are needed (sum over jobs of the beams in use of their scans).  Jobs of a
 * scan without points get a record of zeros.  No NDT in place: NDT2D_ERR_NO_GRID.  A search launched
 * ahead by score_scan is waited out and dropped first.  The NDT stays in place; the beams and the
 * prepared search of the context are not touched.  NDT2D_ERR_INVALID, nothing launched: what
 * refine_scans refuses about jobs and scans. */
int ndt2d_matcher_verify_scans(ndt2d_matcher * m, const double * jobs_xyt, const uint32_t * job_scan,
                               size_t n_jobs, const double * points_xy, const size_t * point_offsets,
                               size_t n_scans, size_t max_beams, uint32_t * records_out,
                               size_t * beam_offsets_out, uint8_t * beam_class_out,
                               double * beam_m2_out, uint32_t * beam_cells_out, size_t beam_cap);
/* The call's object (made by the first verify_scans with an NDT in place; NULL before), for
 * ndt2d_verify_set_timing / _last_ms. */
ndt2d_verify * ndt2d_matcher_verify(ndt2d_matcher * m);
/* The parameters of the later verify_scans calls, kept in the matcher and applied to every call:
 * the neighbourhood (1 or 9; the default at this layer is 9), the gates (each >= 0 and finite;
 * 9.0 and 1.0) and the ray walk (0 or 1; on).  Anything else: NDT2D_ERR_INVALID, the values stay. */
int ndt2d_matcher_set_verify_neighbourhood(ndt2d_matcher * m, uint32_t cells);
int ndt2d_matcher_verify_neighbourhood(ndt2d_matcher * m, uint32_t * out);
int ndt2d_matcher_set_verify_gates(ndt2d_matcher * m, double gate_inlier, double gate_pierce);
int ndt2d_matcher_verify_gates(ndt2d_matcher * m, double * gate_inlier_out, double * gate_pierce_out);
int ndt2d_matcher_set_verify_rays(ndt2d_matcher * m, int enabled);
int ndt2d_matcher_verify_rays(ndt2d_matcher * m, int * out);
/* Newton NDT registration of K jobs, each on a loop-closure candidate's OWN map, in one call
 * (ndt2d_closure_refine on the first device, with the matcher's resolution, range_max and stored
 * scans): what reset() + add_scans_by_id(candidate) + refine_scans(job) gives per job, bit for bit,
 * without the K builds, installs, launches and read-backs -- and without touching the NDT in
 * place: has_ndt and the grid are the same before and after.  Candidates as match_candidates
 * takes them; scans, jobs, job_scan and the outputs as refine_scans takes them; job_candidate[k]:
 * the candidate of job k (NULL: job k uses candidate k, n_jobs must equal n_candidates).  Each
 * scan a job names is subsampled once with laser_max_beams; set_refine_neighbourhood governs this
 * call too.  Jobs of a scan without points: status NO_OVERLAP, score 0.0, their own pose.  A
 * search launched ahead by score_scan is waited out and dropped first.  NDT2D_ERR_INVALID,
 * nothing launched: everything match_candidates refuses about a candidate, everything
 * refine_scans refuses about scans, jobs and rules, a job_candidate out of range ("job k"); a
 * refused call leaves the output arrays as they were. */
int ndt2d_matcher_refine_candidates(ndt2d_matcher * m, const size_t * cand_offsets, const size_t * ids,
                                    const double * poses_xyt, size_t n_candidates,
                                    const double * jobs_xyt, const uint32_t * job_scan,
                                    const uint32_t * job_candidate, size_t n_jobs,
                                    const double * points_xy, const size_t * point_offsets,
                                    size_t n_scans, uint32_t max_evals, double tol_lin, double tol_ang,
                                    double * poses_out, double * scores_out, double * start_scores_out,
                                    double * gradients_out, double * hessians_out, int32_t * status_out,
                                    uint32_t * evals_out);
/* Match verification of K jobs, each on a loop-closure candidate's OWN map, in one call
 * (ndt2d_closure_verify on the first device, with the matcher's resolution, range_max and stored
 * scans): what reset() + add_scans_by_id(candidate) + verify_scans(job) gives per job, bit for bit,
 * without the K builds, installs, launches and read-backs -- and without touching the NDT in
 * place: has_ndt and the grid are the same before and after, and no NDT in place is no error.
 * Candidates and job_candidate as refine_candidates takes them; scans, jobs, job_scan, max_beams,
 * the outputs and beam_cap as verify_scans takes them.  Governed by the matcher's verify
 * parameters (set_verify_neighbourhood, _gates, _rays).  Jobs of a scan without points get a
 * record of zeros.  A search launched ahead by score_scan is waited out and dropped first.
 * NDT2D_ERR_INVALID, nothing launched, the outputs as they were: everything match_candidates
 * refuses about a candidate, everything verify_scans refuses about scans and jobs, a
 * job_candidate out of range ("job k"). */
int ndt2d_matcher_verify_candidates(ndt2d_matcher * m, const size_t * cand_offsets, const size_t * ids,
                                    const double * poses_xyt, size_t n_candidates,
                                    const double * jobs_xyt, const uint32_t * job_scan,
                                    const uint32_t * job_candidate, size_t n_jobs,
                                    const double * points_xy, const size_t * point_offsets,
                                    size_t n_scans, size_t max_beams, uint32_t * records_out,
                                    size_t * beam_offsets_out, uint8_t * beam_class_out,
                                    double * beam_m2_out, uint32_t * beam_cells_out, size_t beam_cap);
/* The two halves of matchScan, for sharded (multi-GPU) searches:
 * prepare_search subsamples the scan (:95-96,110), builds the offset and
 * cos/sin tables (:103-107,117,119) and uploads them -- after it,
 * ndt2d_match_launch(ndt2d_matcher_device(m), th_begin, th_end, ...) evaluates
 * any theta slab; finish_match turns a (combined) NDT2D_MATCH_RECORD_DOUBLES
 * record into matchScan's outputs (:128-134,146,148). */
int ndt2d_matcher_prepare_search(ndt2d_matcher * m, const double * scan_pose_xyt,
                                 const double * points_xy, size_t n_points, size_t * n_th_out,
                                 size_t * n_lin_out, size_t * n_beams_out);
int ndt2d_matcher_finish_match(ndt2d_matcher * m, const double * record, double * pose_inout,
                               double * covariance_out, double * score_out);
/* Subsample + upload the beams only (particle path; then
 * ndt2d_score_poses_launch on ndt2d_matcher_device(m)). */
int ndt2d_matcher_prepare_beams(ndt2d_matcher * m, const double * points_xy, size_t n_points,
                                size_t * n_beams_out);
/* ScanMatcherNDT::scoreScan (:151-154) and scorePoints (:156-178).
 * The mapper calls scoreScan(scan) and then matchScan(scan, ...) (src/ndt_mapper.cpp:514-515,
 * 552-553).  Once a matcher has seen that pair -- a matchScan of the scan and pose of the
 * scoreScan just before it -- its scoreScan queues the scan's search behind the scoring kernel
 * before it waits for the score, and the matchScan that follows collects that search (same
 * kernels, same results; the search starts when the scoring kernel ends instead of a host
 * round trip later).  Any other call waits such a search out, drops it, and the matcher stops
 * launching ahead until it sees the pair again.  ndt2d_matcher_set_search_ahead(m, 0) turns
 * it off (default: on). */
int ndt2d_matcher_score_scan(ndt2d_matcher * m, const double * scan_pose_xyt,
                             const double * points_xy, size_t n_points, double * score_out);
int ndt2d_matcher_set_search_ahead(ndt2d_matcher * m, int enabled);
/* Near-tie adjudication (default: on).  When a search's winner comes back with near_tie set,
 * matchScan lists the candidates within the tolerance of the best (ndt2d_match_near_best with
 * NDT2D_NEAR_TIE_REL, the first 256 in visiting order), rescores each on the host exactly as the reference does (points_outer / points_inner,
 * NDT::likelihood in beam order, libm's exp; src/scan_matcher_ndt.cpp:106-127) and applies the
 * reference's rule -- strict `<` in visiting order (:128-134): the lowest host score, between equal
 * ones the lowest flat index.  The returned pose / score are then that candidate's (the score
 * the reference's own bits); the covariance sums are unaffected.  Needs the host copy of the
 * NDT and of the beams (not available to ndt2d_matcher_match_laser_scan, which skips it).
 * stats: searches that came back marked, and how many of those changed the winner. */
int ndt2d_matcher_set_adjudication(ndt2d_matcher * m, int enabled);
/* The same for a search that was sharded from outside (one process per GPU, ndt_2d_amd/dist.py):
 * record_inout[NDT2D_MATCH_RECORD_DOUBLES] is the COMBINED record of all shards; if its winner
 * is marked (index + 0.5) it is settled as above -- on this matcher's own device, over the whole
 * lattice of the last ndt2d_matcher_prepare_search, which every rank holds: all ranks reach the
 * same verdict without talking to each other -- and leaves with a plain index either way. */
int ndt2d_matcher_settle_near_tie(ndt2d_matcher * m, const double * scan_pose_xyt, double * record_inout);
int ndt2d_matcher_adjudication_stats(ndt2d_matcher * m, uint64_t * marked, uint64_t * changed, uint64_t * truncated);
/* Where ONE pose is scored (scorePoints, scoreScan).  "host" (default): a scan of at most
 * max_beams subsampled beams (default 256; 0 keeps the current value) is scored by the calling
 * thread from the host copy of the NDT, in the reference's order with libm's exp
 * (src/scan_matcher_ndt.cpp:156-178, src/ndt_model.cpp:105-116,162-170,203-218) -- the unchanged
 * ParticleFilter::measure calls scorePoints once per particle (src/particle_filter.cpp:81-87),
 * and a kernel launch plus a PCIe round trip per call costs several times the ~100 cell
 * evaluations it is for (SURVEY.md 8b foresees exactly this path for the per-pose virtual
 * call).  It needs a live matcher -- a GPU -- all the same: searches, batches
 * (ndt2d_matcher_score_poses / _pf_measure) and longer scans always run on the device, and
 * "device" sends the single poses there as well (the parity tests run both and compare). */
int ndt2d_matcher_set_single_pose_path(ndt2d_matcher * m, const char * where, size_t max_beams);
/* Searches launched ahead by scoreScan, and how many of them a matchScan collected. */
int ndt2d_matcher_search_ahead_stats(ndt2d_matcher * m, uint64_t * launched, uint64_t * collected);
int ndt2d_matcher_score_points(ndt2d_matcher * m, const double * points_xy, size_t n_points,
                               const double * pose_xyt, double * score_out);
/* ScanMatcherNDT::reset (:180-183). */
int ndt2d_matcher_reset(ndt2d_matcher * m);
int ndt2d_matcher_has_ndt(ndt2d_matcher * m);

/* laserCallback's LaserScan -> Scan conversion (src/ndt_mapper.cpp:385-453) fused
 * with matchScan: the raw ranges go to the device, where they are converted,
 * de-skewed, subsampled and searched; *n_points_out (optional) = points the
 * conversion kept.  Same outputs and conventions as ndt2d_matcher_match_scan on
 * the converted points. */
int ndt2d_matcher_match_laser_scan(ndt2d_matcher * m, const double * scan_pose_xyt,
                                   const float * ranges, size_t n_ranges,
                                   const ndt2d_laser_scan * scan, double * pose_inout,
                                   double * covariance_out, double * score_out,
                                   size_t * n_points_out);

/* Additive batched interface (not in the reference's ScanMatcher): scores
 * n_poses poses in one launch; scores_out[i] == scorePoints(points, pose_i). */
int ndt2d_matcher_score_poses(ndt2d_matcher * m, const double * points_xy, size_t n_points,
                              const double * poses_xyt, size_t n_poses, double * scores_out);
/* ParticleFilter::measure (src/particle_filter.cpp:78-89) incl. its
 * updateStatistics (:163-218): weights_out[n] = normalised weights,
 * mean_out[3], cov_inout[9] row-major ((2,2) accumulates onto the previous
 * value, :216). */
int ndt2d_matcher_pf_measure(ndt2d_matcher * m, const double * particles_xyt,
                             size_t n_particles, const double * points_xy, size_t n_points,
                             double * weights_out, double * mean_out, double * cov_inout);

/* Host NDT introspection (tests compare it bit-for-bit with the oracle). */
int ndt2d_matcher_grid_info(ndt2d_matcher * m, uint32_t * size_x, uint32_t * size_y,
                            double * cell_size, double * origin_x, double * origin_y);
int ndt2d_matcher_grid_cells6(ndt2d_matcher * m, double * cells6_out, size_t capacity_cells);
/* The search lattice the matcher visits (the reference's FP-accumulated
 * loops): writes up to cap values, returns the count through *n_out. */
int ndt2d_search_offsets(double size, double res, double * out, size_t cap, size_t * n_out);
/* The draw-and-stop loop of ParticleFilter::resample (src/particle_filter.cpp:
 * 94-134), host code.  This is the host form and the parity reference of the
 * device form (ndt2d_resample_launch, section 1), which returns the same indices and
 * count for every input.  Draw i picks the particle whose cumulative weight
 * first exceeds uniforms[i] * sum(weights) (what std::discrete_distribution does
 * with its own generator, :94,110; the caller supplies the uniforms in [0, 1), so
 * any generator can drive it), inserts its KD-tree key
 * static_cast<int>(value / leaf_size3[d]) (kd_tree.hpp:95-98; the leaf count is the
 * number of distinct keys) and recomputes Mx (:117-126); the loop ends when the
 * count reaches max(min_particles, Mx) or max_particles (:107,129-132).
 * indices_out[max_particles] receives the chosen particle of every draw kept,
 * *n_out their number.  n_uniforms must be at least max_particles. */
int ndt2d_kld_resample(const double * particles_xyt, const double * weights, size_t n,
                       size_t min_particles, size_t max_particles, double kld_err, double kld_z,
                       const double * leaf_size3, const double * uniforms, size_t n_uniforms,
                       uint32_t * indices_out, size_t * n_out);
/* Host-only (no GPU needed) NDT build: the arithmetic of addScans without the
 * upload, for hosts that only want the packed grid. */
int ndt2d_host_build_grid(double ndt_resolution, double range_max, const double * poses_xyt,
                          const double * points_xy, const size_t * offsets, size_t n_scans,
                          double * cells6_out, size_t capacity_cells, uint32_t * size_x,
                          uint32_t * size_y, double * origin_x, double * origin_y);
/* ... with flags: NDT2D_BUILD_SEQUENTIAL adds every scan's points one after the other, the
 * reference's loop as it stands (src/ndt_model.cpp:132-152), instead of the four quarters of a
 * scan side by side (csrc/host/ndt2d_host_ndt.cpp HostNdt::add_scan) -- the two give the same bits, and
 * tests/test_host_logic.py holds them to it; NDT2D_BUILD_CLOSED_FORM takes the closed-form
 * eigenvalues (ndt2d_matcher_set_eigenvalue_form "closed").
 *
 * Points off the grid.  Every index of the library -- the host build's two loops, the host
 * single-pose scoring, the device build and every search and pose kernel -- takes a point as
 * outside the grid when
 *   !(x >= origin_x) || !(y >= origin_y) || !(fx < size_x) || !(fy < size_y),
 * fx, fy the double quotients (x - origin) / cell_size, compared before any integer cast.  For a
 * finite point less than 2^32 cells from the origin this is NDT::getIndex (reference
 * src/ndt_model.cpp:203-218) exactly.  A NaN or infinite coordinate, or one 2^32 cells or more
 * away, is outside: there the reference converts an out-of-range double to unsigned int, which is
 * undefined, and this is the one place where the library departs from the literal reference.
 * Such a point adds nothing to a cell and +0.0 to a likelihood (src/ndt_model.cpp:169), as any
 * finite point off the grid does.  The device scorers send it to a sentinel record whose arithmetic
 * would make a NaN or infinite beam NaN, so the matcher layer hands such beams on as finite far
 * points: a beam with a coordinate outside +-1e200 m as (-1e300, -1e300) (csrc/host/ndt2d_host_ndt.cpp
 * subsample_into), and for ndt2d_matcher_match_laser_scan, which converts and subsamples on the
 * device, a kept infinite range as +-FLT_MAX (off_grid_ranges).  The device layer takes its beams as
 * given: a caller of ndt2d_set_beams, ndt2d_set_search_beams or ndt2d_score_poses_beams(_launch)
 * passes beams within +-1e200 m (or far finite stand-ins such as (-1e300, -1e300)); a NaN or
 * infinite beam there scores NaN. */
#define NDT2D_BUILD_SEQUENTIAL 1u
#define NDT2D_BUILD_CLOSED_FORM 2u
int ndt2d_host_build_grid_ex(double ndt_resolution, double range_max, const double * poses_xyt,
                             const double * points_xy, const size_t * offsets, size_t n_scans, unsigned flags,
                             double * cells6_out, size_t capacity_cells, uint32_t * size_x,
                             uint32_t * size_y, double * origin_x, double * origin_y);

/* ------------------------------------------------------------------------ */
/* Synthetic workload generator (BASELINE.md section 3 / SURVEY.md 8d)       */
/* ------------------------------------------------------------------------ */

/* Closed square room [-half, half]^2 with 0.5 m square pillars centred on the
 * lattice (pitch*i + pitch/2, pitch*j + pitch/2) that fit inside the room. */
typedef struct ndt2d_world
{
  double room_half;
  double pillar_pitch;
  double pillar_half;
} ndt2d_world;

/* Ray-cast one n_beams scan over 2*pi (angle_min = -pi) from pose, range noise
 * N(0, noise_sigma^2) from splitmix64(seed) + Box-Muller; writes robot-frame
 * points_xy[2*n_beams]. */
int ndt2d_synth_scan(const ndt2d_world * world, const double * pose_xyt, size_t n_beams,
                     double noise_sigma, uint64_t seed, double * points_xy);
/* 1 if the pose is inside or within `margin` (Chebyshev) of a pillar. */
int ndt2d_synth_pose_blocked(const ndt2d_world * world, double x, double y, double margin);
/* n uniforms in [0,1) from splitmix64(seed). */
int ndt2d_synth_uniform(uint64_t seed, size_t n, double * out);

#ifdef __cplusplus
}
#endif

#endif  /* NDT2D_HIP_H_ */
