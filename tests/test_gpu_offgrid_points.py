"""Points off the grid (include/ndt2d_hip.h, "Points off the grid") through the device build, every
matchScan variant, the single-pose paths, scorePoses, the particle measure and the scan
conversion.  Every result is compared with the oracle on the SUBSTITUTE input -- each NaN, +-inf,
1e300, DBL_MAX or 2^32-cell point replaced by the finite off-grid point (1e6, 1e6), whose fate
the reference defines (tests/offgrid_cases.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import offgrid_cases as G
import oracle_lib as O
from ndt_2d_amd import ScanMatcherNDT, _capi, synth
from ndt_2d_amd.scan_matcher import pf_measure

pytestmark = pytest.mark.gpu

TOL = 1e-12          # scores of a search against the oracle (tests/test_gpu_single_pose_host.py)
TOL_RAW = 1e-9       # raw pose-batch weights (tests/test_gpu_fuzz.py)
SEARCH = dict(search_linear_size=0.03, search_linear_resolution=0.01, search_angular_size=0.02,
              search_angular_resolution=0.01, laser_max_beams=1000)
SCAN_POSE = (0.01, -0.02, 0.005)
MATCH_VARIANTS = ("lane", "lane-noskip", "small", "small-noskip", "wave", "wave-global", "auto", "lds", "global")
POSE_VARIANTS = ("auto", "batched", "compact-exact", "dense")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _setup(name, n, **override):
    cell, range_max = G.MAPS[name]
    orig, subs = G.map_scans(name, n)
    p = dict(ndt_resolution=cell, range_max=range_max, **SEARCH)
    p.update(override)
    ref = O.ScanMatcherNDT()
    ref.initialize(**p)
    ref.addScans(subs)
    gpu = ScanMatcherNDT(0)
    gpu.initialize("offgrid", **p)
    return p, orig, subs, ref, gpu


def _finite_only(orig, subs):
    """The probe scans with their non-finite and DBL_MAX points replaced by the finite off-grid
    ones (1e300, -1e300, the 2^32-cell points): a finite beam reach, so the lane and
    small-lattice searches take it."""
    out = []
    for (pose, pts), (_, sub) in zip(orig, subs):
        pts = pts.copy()
        far = [k for k in range(len(pts)) if G.is_off_grid_value(pts[k:k + 1])[0]]
        finite = [k for k in far if np.isfinite(pts[k]).all() and np.abs(pts[k]).max() < 1e308]
        for i, k in enumerate(far):
            if k not in finite:
                pts[k] = (1e300, -1e300) if i % 2 else (-1e300, 7.0)
        out.append(((pose, pts), (pose, sub)))
    return out


def _check_variants(gpu, query, exp, label):
    ran, exact = [], {}
    for variant in MATCH_VARIANTS:
        gpu.set_variant(variant)
        try:
            got = gpu.matchScan(SCAN_POSE, query, want_scores=True)
        except Exception as e:
            # (the lane mappings refuse a non-finite reach; "lds" a grid that does not fit LDS)
            assert variant.startswith(("lane", "small", "lds")) and "launch_match" in str(e), (label, variant, e)
            continue
        ran.append(variant)
        assert got["n_candidates"] == exp["n_candidates"], (label, variant)
        assert np.array_equal(np.isnan(got["scores"]), np.isnan(exp["scores"])), (label, variant)
        assert np.allclose(got["scores"], exp["scores"], rtol=0, atol=TOL, equal_nan=True), (label, variant)
        assert got["best_index"] == exp["best_index"], (label, variant)
        assert got["score"] == pytest.approx(exp["score"], abs=TOL)
        if variant in ("lane", "small"):
            exact[variant] = got["scores"]
        elif variant.endswith("-noskip") and variant[:-7] in exact:
            assert np.array_equal(_bits(got["scores"]), _bits(exact[variant[:-7]])), (label, variant)
    gpu.set_variant("auto")
    return ran


@pytest.mark.parametrize("n", G.SCAN_LENGTHS)
@pytest.mark.parametrize("name", sorted(G.MAPS))
def test_device_build_is_the_substitutes_grid(name, n):
    cell, range_max = G.MAPS[name]
    p, orig, subs, ref, gpu = _setup(name, n)
    want = _bits(ref.ndt.cells6())
    sx, sy, _, _ = G.geometry(cell, range_max)
    modes = ("device", "host", "auto") if sx * sy * G.HOST_CELL_BYTES > G.SIDE_BY_SIDE_MAX_BYTES else ("device",)
    for mode in modes:
        gpu.set_build_mode(mode)
        gpu.addScans(orig)
        cells, gx, gy, _, ox, oy = gpu.grid()
        assert (gx, gy, ox, oy) == (sx, sy, -range_max, -range_max)
        assert np.array_equal(_bits(cells), want), (name, n, mode)


@pytest.mark.parametrize("n", [33, 720])
@pytest.mark.parametrize("name", sorted(G.MAPS))
def test_match_scan_every_variant(name, n):
    p, orig, subs, ref, gpu = _setup(name, n)
    gpu.addScans(orig)
    probes = list(zip(orig[3:], subs[3:]))
    cases = [("non-finite", probes[0]), ("non-finite", probes[5])] + \
        [("finite", c) for c in _finite_only(orig[3:4] + orig[9:10], subs[3:4] + subs[9:10])]
    for label, ((_, q), (_, qs)) in cases:
        assert G.is_off_grid_value(q).sum() >= 5
        exp = ref.matchScan(SCAN_POSE, qs, want_scores=True)
        assert np.count_nonzero(exp["scores"]) > 0
        ran = _check_variants(gpu, q, exp, (name, n, label))
        assert {"wave", "wave-global", "auto", "global"} <= set(ran)
        if name in ("div-small", "p2-small"):
            assert "lds" in ran, (name, n, label)      # (32 x 32 / 39 x 39 cells: the grid fits LDS)


@pytest.mark.parametrize("reach", [1e6, 1e300])
def test_lane_and_small_searches_clamp_far_beams(reach):
    """A beam of huge finite reach on the 41 x 41 map: the window is the whole grid, the lane and
    small-lattice searches run, and every far beam's fixed-point coordinate is clamped."""
    p = synth.matcher_params(1)
    guess, pts, _ = synth.query_scan(1)
    use = min(p["laser_max_beams"], len(pts))
    step = float(len(pts)) / use
    picked = [int(i * step) for i in range(use)]
    q = pts.copy()
    for j, i in enumerate([0, 1, use // 4, use // 2, use // 2 + 1, use - 1]):
        a = 0.7 * j
        q[picked[i]] = (reach * math.cos(a), reach * math.sin(a))
    ref = O.ScanMatcherNDT()
    ref.initialize(**p)
    ref.addScans(synth.map_scans(1))
    exp = ref.matchScan(guess, q, want_scores=True)
    gpu = ScanMatcherNDT(0)
    gpu.initialize("reach", **p)
    gpu.addScans(synth.map_scans(1))
    assert gpu.grid()[1:3] == (41, 41)
    seen = {}
    for variant in MATCH_VARIANTS:
        gpu.set_variant(variant)
        try:
            got = gpu.matchScan(guess, q, want_scores=True)
        except Exception as e:
            assert reach > 1e6 and variant.startswith(("lane", "small")) and "launch_match" in str(e), (variant, e)
            continue
        seen[variant] = (gpu.last_variant(), got["scores"])
        assert got["n_candidates"] == exp["n_candidates"] == 17640
        assert np.allclose(got["scores"], exp["scores"], rtol=0, atol=1e-9), variant
        assert got["best_index"] == exp["best_index"], variant
    if reach == 1e6:
        assert "lane-per-candidate" in seen["lane"][0], seen["lane"][0]
        assert "small-lattice" in seen["small"][0], seen["small"][0]
    for v in ("lane", "small"):
        if v in seen:
            assert np.array_equal(_bits(seen[v][1]), _bits(seen[v + "-noskip"][1]))
    gpu.set_variant("auto")


@pytest.mark.parametrize("name", ["p2-small", "div-small", "div-large"])
def test_single_pose_paths(name):
    p, orig, subs, ref, gpu = _setup(name, 33)
    gpu.addScans(orig)
    poses = [(0.0, 0.0, 0.0), (0.01, -0.02, 0.003), (-0.03, 0.01, -0.2)]
    for (_, q), (_, qs) in list(zip(orig[3:], subs[3:]))[::3]:
        want = [ref.scorePoints(qs, ps) for ps in poses]
        want_scan = [ref.scoreScan(ps, qs) for ps in poses]
        assert any(w != 0.0 for w in want) and not any(math.isnan(w) for w in want)
        gpu.set_single_pose_path("host", 1024)
        for ps, w, ws in zip(poses, want, want_scan):
            assert _bits([gpu.scorePoints(q, ps)]) == _bits([w])
            assert _bits([gpu.scoreScan(ps, q)]) == _bits([ws])
        gpu.set_single_pose_path("device")
        for ps, w, ws in zip(poses, want, want_scan):
            assert abs(gpu.scorePoints(q, ps) - w) < TOL
            assert abs(gpu.scoreScan(ps, q) - ws) < TOL
    gpu.set_single_pose_path("host")


@pytest.mark.parametrize("name", ["p2-small", "div-fine", "div-large", "p2-large"])
def test_score_poses_few_poses_and_particles(name):
    p, orig, subs, ref, gpu = _setup(name, 33)
    gpu.addScans(orig)
    rng = np.random.default_rng(7)
    poses = np.stack([rng.uniform(-0.2, 0.2, 300), rng.uniform(-0.2, 0.2, 300),
                      rng.uniform(-0.5, 0.5, 300)], axis=1)
    for (_, q), (_, qs) in list(zip(orig[3:], subs[3:]))[::4]:
        w_exp = O.pf_measure(ref, poses, qs)
        assert np.count_nonzero(w_exp) > 20 and not np.isnan(w_exp).any()
        by = {}
        for variant in POSE_VARIANTS:
            gpu.set_variant(variant)
            w = by[variant] = gpu.scorePoses(q, poses)
            assert not np.isnan(w).any(), variant
            assert np.allclose(w, w_exp, rtol=0, atol=TOL_RAW), variant
        assert np.array_equal(_bits(by["batched"]), _bits(by["compact-exact"]))
        gpu.set_variant("auto")
        few = gpu.scorePoses(q, poses[:5])
        assert np.allclose(few, w_exp[:5], rtol=0, atol=TOL_RAW)
        # the kernel-argument path: beams and <= 8 poses as arguments, and its launch / fetch pair.
        # The matcher's few-pose calls above took q as it is; these raw device-layer calls take their
        # beams as given, within +-1e200 m (include/ndt2d_hip.h): q with its off-grid beams as the
        # matcher hands them on
        L = _capi.lib()
        h = gpu.device_handle
        beams = np.ascontiguousarray(q)
        beams[G.is_off_grid_value(beams)] = (-1e300, -1e300)
        ps8 = np.ascontiguousarray(poses[:8])
        one = np.zeros(8)
        assert L.ndt2d_score_poses_beams(h, _capi.dptr(beams), len(beams), _capi.dptr(ps8), 8, _capi.dptr(one)) == 0
        assert np.allclose(one, w_exp[:8], rtol=0, atol=TOL_RAW)
        two = np.zeros(8)
        assert L.ndt2d_score_poses_beams_launch(h, _capi.dptr(beams), len(beams), _capi.dptr(ps8), 8) == 0
        assert L.ndt2d_score_fetch(h, _capi.dptr(two)) == 0
        assert np.array_equal(_bits(one), _bits(two))
        # ParticleFilter::measure with its updateStatistics
        w_gpu, mean_gpu, cov_gpu = pf_measure(gpu, poses, q)
        w_ref, mean_ref, cov_ref = O.pf_update_statistics(poses, w_exp)
        assert np.allclose(w_gpu, w_ref, rtol=1e-9, atol=1e-15)
        assert np.allclose(mean_gpu, mean_ref, rtol=1e-9, atol=1e-12)
        assert np.allclose(cov_gpu, cov_ref, rtol=1e-8, atol=1e-12)


def _same_points(got, want):
    """Kept set and order exact, the non-finite pattern exact (sign of an infinity included),
    finite coordinates within the device sincos's last ulps."""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-12 + 4e-16 * np.abs(want[fin]))


def test_scan_conversion_of_extreme_ranges():
    """-inf ("too close", REP-117), -FLT_MAX, FLT_MAX and subnormal ranges pass the reference's
    filter (src/ndt_mapper.cpp:413,436: NaN and range > range_max only; range_max 1e39 keeps
    FLT_MAX): the conversion keeps them as the oracle does, the fused search's beam reach is +inf
    when a kept point is not finite, and the fused matchScan is the oracle's on the substitute."""
    import torch
    fmax = float(np.finfo(np.float32).max)
    sub = float(np.finfo(np.float32).smallest_subnormal)
    guess, pts, _ = synth.query_scan(1)
    n = len(pts)
    ranges = np.hypot(pts[:, 0], pts[:, 1]).astype(np.float32)
    a0 = math.atan2(pts[0, 1], pts[0, 0])
    inc = (math.atan2(pts[1, 1], pts[1, 0]) - a0) % (2 * math.pi)
    special = [-np.inf, -fmax, fmax, sub, -sub, np.inf, np.nan, 4 * sub]
    for j, k in enumerate([0, 1, n // 4 - 1, n // 4, n // 2, n - 2, n - 1, 3 * n // 4]):
        ranges[k] = special[j]
    p = synth.matcher_params(1)
    m = ScanMatcherNDT(0)
    m.initialize("conv", **p)
    ref = O.ScanMatcherNDT()
    ref.initialize(**p)
    ref.addScans(synth.map_scans(1))
    m.addScans(synth.map_scans(1))
    # (range_max inf: +inf is kept as well; 1e39: FLT_MAX is kept, +inf dropped; 10: both dropped)
    for angle_min, increment, rmax in ((0.0, 0.0, 1e39), (a0, inc, 1e39), (a0, inc, 10.0), (a0, inc, np.inf)):
        for inverted in (False, True):
            want = O.convert_scan(ranges, angle_min, increment, rmax, inverted=inverted)
            got = m.convertScan(ranges, angle_min, increment, rmax, inverted=inverted)
            _same_points(got, want)
            if angle_min == 0.0:
                # (exact: every value, and NaN where the oracle has NaN -- whose sign bit IEEE leaves open)
                assert np.array_equal(got, want, equal_nan=True)
        # (-inf passes every range_max)
        assert not np.isfinite(O.convert_scan(ranges, angle_min, increment, rmax)).all()
        # the device's {count, reach bound}
        d_r = torch.from_numpy(ranges).cuda()
        d_p = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        d_i = torch.zeros(2, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        desc = m._laser_scan(angle_min, increment, rmax, False, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        assert _capi.lib().ndt2d_convert_scan_launch(m.device_handle, d_r.data_ptr(), n, C.byref(desc),
                                                     d_p.data_ptr(), d_i.data_ptr()) == _capi.OK
        m.synchronize()
        info = d_i.cpu().numpy()
        want = O.convert_scan(ranges, angle_min, increment, rmax)
        assert int(info[0]) == len(want)
        assert info[1] == np.inf
        # the oracle's matchScan on the converted points is its matchScan on the substitute
        exp = ref.matchScan(guess, want, want_scores=True)
        exp_sub = ref.matchScan(guess, G.substitute(want, G.is_off_grid_value(want)), want_scores=True)
        assert _bits([exp["score"]]) == _bits([exp_sub["score"]]) and not math.isnan(exp["score"])
        assert np.array_equal(_bits(exp["scores"]), _bits(exp_sub["scores"]))
        # ... and so are matchScan's on the device from the same points, and the fused conversion +
        # search's from the ranges themselves (-inf, +inf and NaN included), in every variant
        got = m.matchScan(guess, want)
        assert got["score"] == pytest.approx(exp["score"], abs=1e-9)
        assert np.array_equal(got["pose"], exp["pose"])
        for variant in ("auto", "lane", "small", "wave"):
            m.set_variant(variant)
            try:
                got = m.matchLaserScan(guess, ranges, angle_min, increment, rmax)
            except Exception as e:
                assert variant in ("lane", "small") and "launch_match" in str(e), (variant, e)
                continue
            assert got["n_points"] == len(want)
            assert not math.isnan(got["score"]), variant
            assert got["score"] == pytest.approx(exp["score"], abs=1e-9), variant
            assert np.array_equal(got["pose"], exp["pose"]), variant
        m.set_variant("auto")
