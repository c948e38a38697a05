"""GPU parity for the particle-filter steps either side of `measure`
(SURVEY.md 8(f) row N3): MotionModel::sample, ParticleFilter::init / update /
updateStatistics through the C-ABI against the oracle on the same noise.

Tolerances: theta goes through exact double adds and an exact fmod, so it is
compared bit-for-bit; x / y differ by the device sincos's last ulps (1e-12
absolute bound); statistics by summation order (1e-11 relative)."""
import ctypes as C
import math

import numpy as np
import pytest

import noise_restatement as R
import oracle_lib as O
from ndt_2d_amd import ScanMatcherNDT, _capi, synth
from ndt_2d_amd.particle_filter import MotionModel, ParticleFilter
from ndt_2d_amd.scan_matcher import pf_update

pytestmark = pytest.mark.gpu

ALPHAS = [0.1, 0.1, 0.1, 0.1, 0.0]   # reference test/particle_tests.cpp:76-77
ALPHAS2 = [0.2, 0.05, 0.15, 0.02, 0.0]
MOTIONS = [(1.0, 0.0, 0.0), (0.0, 0.0, 1.57), (0.0, 0.0, -1.57), (0.01, -0.01, 1.57),
           (-0.4, 0.3, 0.2), (0.005, 0.005, -0.3), (2.5, -1.5, 3.0), (0.0, 0.0, 0.0)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def matcher():
    m = ScanMatcherNDT(0)
    m.initialize("pf", **synth.matcher_params(1))
    return m


def _stream(torch, matcher):
    s = torch.cuda.Stream()
    matcher.set_stream(s.cuda_stream)
    return s


def _device_noise(torch, matcher, seed, step, first, n):
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        z = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    matcher.pf_noise_launch(seed, step, first, n, z.data_ptr())
    matcher.synchronize()
    return z


def _random_poses(rng, n):
    p = rng.uniform(-10.0, 10.0, size=(n, 3))
    p[:, 2] = rng.uniform(-np.pi, np.pi, size=n)
    return p


@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("alphas", [ALPHAS, ALPHAS2])
def test_motion_model_given_noise_matches_oracle(torch, matcher, motion, alphas):
    rng = np.random.default_rng(hash((motion, tuple(alphas))) % (2 ** 32))
    n = 5000
    poses = _random_poses(rng, n)
    z = rng.standard_normal((n, 3)).astype(np.float32)
    want, _ = O.motion_sample(*motion, alphas, poses, z)
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(poses).cuda()
        d_z = torch.from_numpy(z).cuda()
    s.synchronize()
    matcher.pf_motion_launch(d_p.data_ptr(), n, *motion, alphas, d_z.data_ptr())
    matcher.synchronize()
    got = d_p.cpu().numpy()
    assert np.array_equal(got[:, 2], want[:, 2])
    assert np.max(np.abs(got[:, :2] - want[:, :2])) < 1e-12


def test_motion_model_philox_path_equals_its_published_noise(torch, matcher):
    """The fused launch draws exactly the numbers ndt2d_pf_noise_launch writes, so
    the oracle fed with them reproduces the device result."""
    n, seed, step = 40000, 0xC0FFEE12345, 7
    poses = _random_poses(np.random.default_rng(3), n)
    z = _device_noise(torch, matcher, seed, step, 0, n).cpu().numpy()
    want, _ = O.motion_sample(0.5, -0.2, 0.4, ALPHAS, poses, z)
    d_p = torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()
    matcher.pf_motion_launch(d_p.data_ptr(), n, 0.5, -0.2, 0.4, ALPHAS, None, seed, step, 0)
    matcher.synchronize()
    got = d_p.cpu().numpy()
    assert np.array_equal(got[:, 2], want[:, 2])
    assert np.max(np.abs(got[:, :2] - want[:, :2])) < 1e-12
    # the same call again is the same draw; another step is another draw
    d_q = torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()
    matcher.pf_motion_launch(d_q.data_ptr(), n, 0.5, -0.2, 0.4, ALPHAS, None, seed, step, 0)
    matcher.synchronize()
    assert torch.equal(d_p, d_q)
    d_r = torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()
    matcher.pf_motion_launch(d_r.data_ptr(), n, 0.5, -0.2, 0.4, ALPHAS, None, seed, step + 1, 0)
    matcher.synchronize()
    assert not torch.equal(d_p, d_r)


def test_noise_stream_is_shard_invariant(torch, matcher):
    """Counter = global particle index: two half launches draw what one whole launch does."""
    n, seed, step = 10001, 99, 3
    whole = _device_noise(torch, matcher, seed, step, 0, n).cpu().numpy()
    cut = 4097
    a = _device_noise(torch, matcher, seed, step, 0, cut).cpu().numpy()
    b = _device_noise(torch, matcher, seed, step, cut, n - cut).cpu().numpy()
    assert np.array_equal(whole, np.concatenate([a, b]))
    # 64-bit indices and seeds are honoured
    far = _device_noise(torch, matcher, seed, step, (1 << 40), 16).cpu().numpy()
    assert not np.array_equal(far, whole[:16])
    other = _device_noise(torch, matcher, seed + (1 << 33), step, 0, 16).cpu().numpy()
    assert not np.array_equal(other, whole[:16])


def test_noise_stream_is_standard_normal(torch, matcher):
    n = 1 << 21
    z = _device_noise(torch, matcher, 2024, 1, 0, n).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(z))
    se = 1.0 / np.sqrt(n)
    assert np.all(np.abs(z.mean(axis=0)) < 5 * se)
    assert np.all(np.abs(z.var(axis=0) - 1.0) < 5 * np.sqrt(2.0) * se)
    assert np.all(np.abs((z ** 3).mean(axis=0)) < 5 * np.sqrt(15.0) * se)
    assert np.all(np.abs((z ** 4).mean(axis=0) - 3.0) < 5 * np.sqrt(96.0) * se)
    # the three draws of a particle are uncorrelated, and so are neighbours
    c = np.corrcoef(z.T)
    assert np.all(np.abs(c - np.eye(3)) < 5 * se)
    assert abs(np.corrcoef(z[:-1, 0], z[1:, 0])[0, 1]) < 5 * se
    # tails: 24-bit uniforms reach |z| ~ 5.7
    assert 4.5 < np.abs(z).max() < 6.0


def test_reference_particle_scenario_on_device(torch, matcher):
    """reference test/particle_tests.cpp:74-140 with the device's own noise stream:
    50 poses, MotionModel(0.1, 0.1, 0.1, 0.1, 0.0), its tolerances.  The scenario is a
    single random draw whose last expectation lies ~3 sigma off the model's true
    mean (tests/test_particle_host.py), so ~3/4 of all seeds satisfy it in the
    reference as well; 24 seeds are run and at least 14 must pass every tolerance."""

    def scenario(seed):
        step = [0]
        ok = [True]

        def sample(d_p, dx, dy, dth):
            step[0] += 1
            matcher.pf_motion_launch(d_p.data_ptr(), 50, dx, dy, dth, ALPHAS, None, seed,
                                     step[0], 0)
            matcher.synchronize()
            return d_p.cpu().numpy().mean(axis=0)

        def zeros():
            p = torch.zeros((50, 3), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            return p

        def near(m, expect, tol):
            ok[0] = ok[0] and bool(np.all(np.abs(m - np.array(expect)) < tol))

        near(sample(zeros(), 1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.3)
        for sign in (1.0, -1.0):
            p = zeros()
            near(sample(p, 0.0, 0.0, sign * 1.57), (0.0, 0.0, sign * 1.57), 0.3)
            near(sample(p, 1.0, 0.0, 0.0), (0.0, sign * 1.0, sign * 1.57), 0.3)
            near(sample(p, 1.0, 0.0, 0.0), (0.0, sign * 2.0, sign * 1.57), 0.5)
            near(sample(zeros(), 0.01, -0.01, sign * 1.57), (0.0, 0.0, sign * 1.57), 0.3)
        return ok[0]

    passed = sum(scenario(seed) for seed in range(1, 25))
    assert passed >= 14, passed


def test_pf_init_matches_oracle(torch, matcher):
    n, seed, step = 30000, 5, 11
    z = _device_noise(torch, matcher, seed, step, 0, n)
    args = (1.25, -3.5, 3.0, 0.3, 0.2, 0.5)   # theta near pi: the wrap is exercised
    want = O.pf_init(*args, z.cpu().numpy())
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        d_a = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        d_b = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    matcher.pf_init_launch(d_a.data_ptr(), n, *args, z.data_ptr())
    matcher.pf_init_launch(d_b.data_ptr(), n, *args, None, seed, step, 0)
    matcher.synchronize()
    assert np.array_equal(d_a.cpu().numpy(), want)
    assert np.array_equal(d_b.cpu().numpy(), want)
    assert (want[:, 2] < 0).any() and (want[:, 2] > 0).any()


@pytest.mark.parametrize("uniform", [False, True])
def test_pose_moments_and_finalize_match_update_statistics(torch, matcher, uniform):
    rng = np.random.default_rng(17)
    n = 70001
    poses = _random_poses(rng, n)
    poses[:, :2] = rng.normal([2.0, -1.0], [0.3, 0.6], size=(n, 2))
    # headings around 3.0 rad straddle the +-pi wrap
    poses[:, 2] = [O.lib().orc_normalize_angle(t) for t in rng.normal(3.0, 0.4, size=n)]
    w = np.full(n, 1.0 / n) if uniform else rng.uniform(0.1, 2.0, size=n)
    cov_prev = np.zeros((3, 3))
    cov_prev[2, 2] = 0.125
    w_want, mean_want, cov_want = O.pf_update_statistics(poses, w, cov_prev)
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(poses).cuda()
        d_w = torch.from_numpy(w).cuda()
        d_s = torch.zeros(16, dtype=torch.float64, device="cuda")
    s.synchronize()
    matcher.pose_moments_launch(d_p.data_ptr(), n, None if uniform else d_w.data_ptr(),
                                d_s.data_ptr())
    matcher.pf_finalize_launch(d_p.data_ptr(), n, d_w.data_ptr(), d_s.data_ptr(),
                               d_s.data_ptr() + 64)
    matcher.synchronize()
    out = d_s.cpu().numpy()[8:]
    assert np.allclose(d_w.cpu().numpy(), w_want, rtol=1e-12, atol=0)
    assert np.allclose(out[1:4], mean_want, rtol=1e-11, atol=1e-13)
    assert np.allclose([out[4], out[5], out[6]],
                       [cov_want[0, 0], cov_want[0, 1], cov_want[1, 1]], rtol=1e-8, atol=1e-12)
    assert cov_prev[2, 2] + out[7] == pytest.approx(cov_want[2, 2], rel=1e-11)


@pytest.mark.parametrize("with_noise", [True, False])
def test_pf_update_host_entry_matches_oracle(torch, matcher, with_noise):
    """ndt2d_pf_update = ParticleFilter::update (motion model + updateStatistics)."""
    rng = np.random.default_rng(23)
    n, seed, step = 12345, 77, 4
    poses = _random_poses(rng, n)
    w = rng.uniform(0.5, 1.5, size=n)
    if with_noise:
        z = rng.standard_normal((n, 3)).astype(np.float32)
    else:
        z = _device_noise(torch, matcher, seed, step, 0, n).cpu().numpy()
    p_want, _ = O.motion_sample(0.3, 0.1, -0.2, ALPHAS2, poses, z)
    w_want, mean_want, cov_want = O.pf_update_statistics(p_want, w)
    p_got, w_got, mean_got, cov_got = pf_update(matcher, poses, w, 0.3, 0.1, -0.2, ALPHAS2,
                                                noise=z if with_noise else None, seed=seed,
                                                step=step)
    assert np.array_equal(p_got[:, 2], p_want[:, 2])
    assert np.max(np.abs(p_got[:, :2] - p_want[:, :2])) < 1e-12
    assert np.allclose(w_got, w_want, rtol=1e-12, atol=0)
    assert np.allclose(mean_got, mean_want, rtol=1e-10, atol=1e-12)
    assert np.allclose(cov_got, cov_want, rtol=1e-8, atol=1e-11)


def test_pf_entry_points_reject_bad_arguments(matcher):
    L = _capi.lib()
    h = matcher.device_handle
    a = (C.c_double * 5)(*ALPHAS)
    assert L.ndt2d_pf_motion_launch(h, None, 10, 0.0, 0.0, 0.0, a, None, 0, 0, 0) == _capi.ERR_INVALID
    assert L.ndt2d_pf_motion_launch(h, 1, 0, 0.0, 0.0, 0.0, a, None, 0, 0, 0) == _capi.ERR_INVALID
    assert L.ndt2d_pf_init_launch(h, None, 10, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None, 0, 0, 0) == _capi.ERR_INVALID
    assert L.ndt2d_pf_noise_launch(h, 0, 0, 0, 10, None) == _capi.ERR_INVALID
    assert L.ndt2d_pose_moments_launch(h, None, 10, None, None) == _capi.ERR_INVALID
    assert b"bad argument" in L.ndt2d_last_error(h)


def test_particle_filter_cycle_matches_oracle(torch):
    """init -> update -> measure -> resample -> update on the device-resident filter
    against the oracle driven with the filter's own (published) noise."""
    cfg = 3
    scans = synth.map_scans(cfg)
    params = synth.matcher_params(cfg)
    gpu = ScanMatcherNDT(0)
    gpu.initialize("pf", **params)
    gpu.addScans(scans)
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans(scans)
    guess, pts, _ = synth.query_scan(cfg)

    n, seed = 3000, 31337
    pf = ParticleFilter(n, 5000, MotionModel(*ALPHAS2), gpu, seed=seed)
    assert np.array_equal(pf.getMean(), np.zeros(3))
    assert np.allclose(pf.getCovariance(), 0.0, atol=1e-30)

    def noise(step, count):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            z = torch.empty((count, 3), dtype=torch.float32, device="cuda")
        s.synchronize()
        gpu.pf_noise_launch(seed, step, 0, count, z.data_ptr())
        gpu.synchronize()
        return z.cpu().numpy()

    cov = np.zeros((3, 3))

    def check(p_want, w_raw):
        nonlocal cov
        w_want, mean_want, cov = O.pf_update_statistics(p_want, w_raw, cov)
        assert np.allclose(pf.getMean(), mean_want, rtol=1e-10, atol=1e-12)
        assert np.allclose(pf.getCovariance(), cov, rtol=1e-8, atol=1e-11)
        got = pf.particles.cpu().numpy()
        assert np.array_equal(got[:, 2], p_want[:, 2])
        assert np.max(np.abs(got[:, :2] - p_want[:, :2])) < 1e-12
        assert np.allclose(pf.weights.cpu().numpy(), w_want, rtol=1e-9, atol=0)
        return w_want

    # init around the query pose (reference src/ndt_mapper.cpp uses 0.1 / 0.1 / 0.1 style sigmas)
    pf.init(guess[0], guess[1], guess[2], 0.15, 0.15, 0.1)
    p = O.pf_init(guess[0], guess[1], guess[2], 0.15, 0.15, 0.1, noise(1, n))
    w = check(p, np.full(n, 1.0 / n))

    pf.update(0.05, 0.01, 0.02)
    p, _ = O.motion_sample(0.05, 0.01, 0.02, ALPHAS2, p, noise(2, n))
    w = check(p, w)

    pf.measure(gpu, pts)
    w = check(p, O.pf_measure(ref, p, pts))
    assert np.all(w > 0) and abs(w.sum() - 1.0) < 1e-12

    before = pf.particles.cpu().numpy()
    pf.resample(0.01, 0.99)
    m = len(pf.particles)
    assert n <= m <= 5000
    got = pf.particles.cpu().numpy()
    # every survivor is one of the previous particles, carrying its weight (:112-116)
    order = {tuple(row): i for i, row in enumerate(before)}
    idx = np.array([order[tuple(row)] for row in got])
    w_norm, mean_want, cov = O.pf_update_statistics(p[idx], w[idx], cov)
    assert np.allclose(pf.weights.cpu().numpy(), w_norm, rtol=1e-9, atol=0)
    assert np.allclose(pf.getMean(), mean_want, rtol=1e-10, atol=1e-12)
    assert np.allclose(pf.getCovariance(), cov, rtol=1e-8, atol=1e-11)
    # heavier particles are drawn more often
    counts = np.bincount(idx, minlength=n)
    assert np.corrcoef(counts, w)[0, 1] > 0.08

    pf.update(0.02, 0.0, -0.01)
    p2, _ = O.motion_sample(0.02, 0.0, -0.01, ALPHAS2, p[idx], noise(3, m))
    check(p2, w_norm)
    msg = pf.getMsg()
    assert msg.shape == (m, 4) and np.allclose(msg[:, 2] ** 2 + msg[:, 3] ** 2, 1.0)


def test_eight_wave_groups_give_the_four_wave_bits():
    """Particle sets too small to fill the chip put EIGHT waves on each group of 64 particles
    (512-thread blocks, one chunk of the beams per wave) instead of four: the weights and the
    statistics must not depend on it (ndt2d_poses_compact.hip, poses_eight_wave_groups)."""
    import os
    from ndt_2d_amd import ScanMatcherNDT, pf_measure, synth
    m = ScanMatcherNDT(0)
    m.initialize("pf", **synth.matcher_params(3))
    m.addScans(synth.map_scans(3))
    _, pts, _ = synth.query_scan(3)
    parts = synth.particles(3, 20000)
    out = {}
    for knob in ("0", "1"):
        os.environ["NDT2D_POSES_EIGHT_WAVES"] = knob
        try:
            out[knob] = (m.scorePoses(pts, parts), pf_measure(m, parts, pts))
        finally:
            del os.environ["NDT2D_POSES_EIGHT_WAVES"]
    assert np.array_equal(out["0"][0], out["1"][0])
    assert np.count_nonzero(out["0"][0]) > 1000
    for a, b in zip(out["0"][1], out["1"][1]):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-15)       # (the moment sums meet in another order)
    auto = m.scorePoses(pts, parts)                              # the policy's own choice: the same bits
    assert np.array_equal(auto, out["0"][0])


# ---- the noise stream against its CPU restatement ---------------------------------------------
#
# tests/noise_restatement.py restates the stream from the header's words (Philox4x32-10, the
# float32 uniform, Box-Muller) and is itself pinned to the Random123 known answers on the CPU
# (tests/test_noise_restatement.py).  The device's float32 normals are held to its float64 ones.

# Maximum errors of the device's logf and sinf / cosf in ulp.  The ROCm installs this was written
# against carry no copy of the HIP math API's accuracy table, so 2 ulp is taken for each.
E_LOG_ULP = 2
E_TRIG_ULP = 2
NOISE_B = E_LOG_ULP + 1 + 2 * E_TRIG_ULP + 1          # = 8, see _noise_ratio

# the grid cap of the streaming kernels (kMaxStreamBlocks, kMaxPosesBlocks) and their block size
CAP_BLOCKS, BLOCK = 4096, 256
# the smallest size that sends some threads round their loop again AND leaves a partial wave
N_BEYOND = CAP_BLOCKS * BLOCK + 257
SMALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511)

KAT_STREAM = R.KAT_STREAM          # (seed, step, first) forms of the Random123 known answers
R_MAX = R.R_MAX                    # sqrt(-2 log 2^-25) = 5.8870501...


def _noise(torch, matcher, seed, step, first, n):
    """ndt2d_pf_noise_launch into a buffer that held NaN: what is not written stays visible."""
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        z = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    s.synchronize()
    matcher.pf_noise_launch(seed, step, first, n, z.data_ptr())
    matcher.synchronize()
    return z


def _noise_ratio(z_dev, seed, step, first):
    """max |z_dev - z_ref| / (2^-24 max(1, r)) over the components, r the component's radius.

    The bound on it, in units of 2^-24 max(1, r), term by term for z = r * trig(a), where the
    uniforms and the float32 angle a are reproduced to the bit (so the arguments carry no error):
      * logf: E_LOG_ULP ulp; an ulp is at most 2^-23 of the value, so the relative error of
        -2 log u is at most 2 E_LOG_ULP 2^-24, and the square root halves it:     E_LOG_ULP
      * sqrtf is correctly rounded, half an ulp <= 2^-24 relative:                 1
      * cosf / sinf: E_TRIG_ULP ulp of a value of magnitude <= 1, an ulp there at most 2^-23,
        i.e. 2 E_TRIG_ULP 2^-24 absolute, times r:                                 2 E_TRIG_ULP
      * the product r * trig is correctly rounded, 2^-24 relative, |z| <= r:       1
    NOISE_B = E_LOG_ULP + 1 + 2 E_TRIG_ULP + 1 = 8 (2.8e-6 at the largest radius), second-order
    terms dropped (they are 2^-24 times smaller).  numpy's float32 chain measures 2.9 on the CPU.
    Largest ratio observed on an MI355X over every case of this file: 3.16 (beyond the cap,
    n = 1,048,833; 3.10 at n = 20001)."""
    z_dev = np.asarray(z_dev, dtype=np.float64)
    assert np.all(np.isfinite(z_dev))
    z_ref, r = R.normals_reference(seed, step, first, len(z_dev))
    ratio = np.abs(z_dev - z_ref) / (2.0 ** -24 * np.maximum(1.0, r))
    return float(ratio.max())


@pytest.mark.parametrize("seed,step,first,n", [
    (0xC0FFEE12345, 7, 0, 20001),
    (0xC0FFEE12345, 7, 4097, 1000),
    (0xC0FFEE12345, 7, (1 << 40) + 3, 64),
    (0xC0FFEE12345, (5 << 32) + 9, 0, 1000),
    (99 + (1 << 33), 7, 0, 1000),
] + [(seed, step, first, 1) for seed, step, first in KAT_STREAM])
def test_noise_stream_is_the_restatement(torch, matcher, seed, step, first, n):
    """Every word of (seed, step, index) is where the header says: wrong round constants, swapped
    counter words, a dropped high half, cos / sin or w[1] / w[2] exchanged all move a draw by
    O(1), the bound is NOISE_B 2^-24 max(1, r) (derived at _noise_ratio).  The last three cases
    are single draws whose counter and key are the three Random123 known-answer vectors."""
    z = _noise(torch, matcher, seed, step, first, n).cpu().numpy()
    ratio = _noise_ratio(z, seed, step, first)
    print("noise ratio (seed=%#x step=%#x first=%#x n=%d): %.3f" % (seed, step, first, n, ratio))
    assert ratio <= NOISE_B, ratio


def test_noise_sub_range_is_the_slice_of_the_restated_whole(torch, matcher):
    seed, step = 0xC0FFEE12345, 7
    whole = _noise(torch, matcher, seed, step, 0, 20001).cpu().numpy()
    part = _noise(torch, matcher, seed, step, 4097, 1000).cpu().numpy()
    assert np.array_equal(part, whole[4097:5097])


# seed = 1, step = 1: the particle indices whose words have all-ones / all-zero top 24 bits
# (tests/test_noise_restatement.py asserts the words)
D_SEED, D_STEP = R.DESIGNED_SEED, R.DESIGNED_STEP
D_UR_ONE, D_UR_MIN, D_UR2_ONE, D_UR2_MIN, D_UA_ONE, D_UA_MIN = (
    R.D_UR_ONE, R.D_UR_MIN, R.D_UR2_ONE, R.D_UR2_MIN, R.D_UA_ONE, R.D_UA_MIN)


def test_designed_draws_at_the_ends_of_the_uniform(torch, matcher):
    """The uniform is float32 RNE of (k + 0.5) times 2^-24, in (0, 1]: k = 2^24 - 1 gives 1.0f,
    radius 0 and exactly zero normals; k = 0 gives the largest radius, sqrt(50 ln 2)."""
    got = {}
    for index in (D_UR_ONE, D_UR_MIN, D_UR2_ONE, D_UR2_MIN, D_UA_ONE, D_UA_MIN):
        z = _noise(torch, matcher, D_SEED, D_STEP, index, 1).cpu().numpy()
        assert np.all(np.isfinite(z)), (index, z)
        ratio = _noise_ratio(z, D_SEED, D_STEP, index)
        print("designed draw %d: z = %r ratio %.3f" % (index, z[0].tolist(), ratio))
        assert ratio <= NOISE_B, (index, ratio)
        got[index] = z[0].astype(np.float64)
    assert got[D_UR_ONE][0] == 0.0 and got[D_UR_ONE][1] == 0.0        # (either sign of zero)
    assert got[D_UR2_ONE][2] == 0.0
    tol = NOISE_B * 2.0 ** -24 * R_MAX
    # (two components, each within tol of the reference's: their hypot within sqrt(2) tol)
    assert abs(np.hypot(got[D_UR_MIN][0], got[D_UR_MIN][1]) - R_MAX) <= math.sqrt(2.0) * tol
    _, r = R.normals_reference(D_SEED, D_STEP, D_UR2_MIN, 1)
    assert r[0, 2] == pytest.approx(R_MAX, rel=1e-15, abs=0)
    z_ref, _ = R.normals_reference(D_SEED, D_STEP, D_UR2_MIN, 1)
    assert abs(got[D_UR2_MIN][2] - z_ref[0, 2]) <= tol
    # angle = float32 2 pi and the smallest angle: the cosine is 1 to the bound, the sine tiny
    for index in (D_UA_ONE, D_UA_MIN):
        z_ref, r = R.normals_reference(D_SEED, D_STEP, index, 1)
        assert z_ref[0, 0] == pytest.approx(r[0, 0], rel=1e-12, abs=0) and abs(z_ref[0, 1]) < 1e-6 * r[0, 0]


def test_motion_on_the_zero_radius_draw_matches_oracle(torch, matcher):
    """The fused Philox path at the index whose radius is 0: the oracle with z = (0, 0, z2)."""
    z = _noise(torch, matcher, D_SEED, D_STEP, D_UR_ONE, 1).cpu().numpy()
    z_ref, _ = R.normals_reference(D_SEED, D_STEP, D_UR_ONE, 1)
    z_want = np.array([[0.0, 0.0, z[0, 2]]], dtype=np.float32)
    assert abs(float(z[0, 2]) - z_ref[0, 2]) <= NOISE_B * 2.0 ** -24 * max(1.0, abs(z_ref[0, 2]))
    poses = np.array([[1.25, -0.5, 0.75]])
    for motion, alphas in ((MOTIONS[4], ALPHAS2), (MOTIONS[6], ALPHAS)):
        want, _ = O.motion_sample(*motion, alphas, poses, z_want)
        got = _motion(torch, matcher, poses, motion, alphas, None, D_SEED, D_STEP, D_UR_ONE)
        assert np.array_equal(got[:, 2], want[:, 2])
        assert np.max(np.abs(got[:, :2] - want[:, :2])) < 1e-12
        assert not np.array_equal(got, poses)


# ---- the streaming kernels at the sizes where their loops and reductions change shape ----------

def _motion(torch, matcher, poses, motion, alphas, z=None, seed=0, step=0, first=0):
    n = len(poses)
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).cuda()
        d_z = None if z is None else torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).cuda()
    s.synchronize()
    matcher.pf_motion_launch(d_p.data_ptr(), n, *motion, alphas,
                             None if d_z is None else d_z.data_ptr(), seed, step, first)
    matcher.synchronize()
    return d_p.cpu().numpy()


def _init(torch, matcher, n, args, z=None, seed=0, step=0, first=0):
    """ndt2d_pf_init_launch into poses that held -1.0e30 (no init result is that)."""
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        d_p = torch.full((n, 3), -1.0e30, dtype=torch.float64, device="cuda")
        d_z = None if z is None else torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).cuda()
    s.synchronize()
    matcher.pf_init_launch(d_p.data_ptr(), n, *args, None if d_z is None else d_z.data_ptr(),
                           seed, step, first)
    matcher.synchronize()
    return d_p.cpu().numpy()


def _statistics(torch, matcher, poses, w, uniform):
    """pose_moments_launch + pf_finalize_launch: (the eight raw sums, out[8], weights)."""
    n = len(poses)
    s = _stream(torch, matcher)
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).cuda()
        d_w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
        d_s = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    s.synchronize()
    matcher.pose_moments_launch(d_p.data_ptr(), n, None if uniform else d_w.data_ptr(),
                                d_s.data_ptr())
    matcher.pf_finalize_launch(d_p.data_ptr(), n, d_w.data_ptr(), d_s.data_ptr(),
                               d_s.data_ptr() + 64)
    matcher.synchronize()
    st = d_s.cpu().numpy()
    return st[:8].copy(), st[8:].copy(), d_w.cpu().numpy()


def _wrap_poses(rng, n):
    """The particle cloud of test_pose_moments_and_finalize_match_update_statistics: headings
    around 3.0 rad straddle the +-pi wrap."""
    poses = np.empty((n, 3))
    poses[:, :2] = rng.normal([2.0, -1.0], [0.3, 0.6], size=(n, 2))
    t = rng.normal(3.0, 0.4, size=n)
    poses[:, 2] = np.where(t > np.pi, t - 2.0 * np.pi, t)
    assert np.all(np.abs(poses[:, 2]) <= np.pi)
    return poses


def _check_statistics(poses, w, out, w_got, tail=None):
    """Against ParticleFilter::updateStatistics at the tolerances of
    test_pose_moments_and_finalize_match_update_statistics."""
    cov_prev = np.zeros((3, 3))
    cov_prev[2, 2] = 0.125
    w_want, mean_want, cov_want = O.pf_update_statistics(poses, w, cov_prev)
    assert np.allclose(w_got, w_want, rtol=1e-12, atol=0)
    assert np.allclose(out[1:4], mean_want, rtol=1e-11, atol=1e-13)
    assert np.allclose([out[4], out[5], out[6]],
                       [cov_want[0, 0], cov_want[0, 1], cov_want[1, 1]], rtol=1e-8, atol=1e-12)
    assert cov_prev[2, 2] + out[7] == pytest.approx(cov_want[2, 2], rel=1e-11)
    if tail is not None:
        assert np.allclose(w_got[-tail:], (np.asarray(w) / np.sum(w))[-tail:], rtol=1e-12, atol=0)
        if abs(np.sum(w) - 1.0) > 1e-3:
            assert np.all(w_got[-tail:] != np.asarray(w)[-tail:])   # normalised in place


def _check_motion_and_init(torch, matcher, n, rng, seed, step, first, z_dev, tail=None):
    """motion_kernel and init_kernel, with given noise and on the Philox path, against the
    oracle: theta bit for bit, x / y < 1e-12."""
    poses = _random_poses(rng, n)
    z = rng.standard_normal((n, 3)).astype(np.float32)
    motion, alphas = MOTIONS[4], ALPHAS2
    for noise, kw in ((z, {}), (z_dev, dict(seed=seed, step=step, first=first))):
        want, _ = O.motion_sample(*motion, alphas, poses, noise)
        got = _motion(torch, matcher, poses, motion, alphas, None if kw else noise, **kw)
        assert np.array_equal(got[:, 2], want[:, 2])
        assert np.max(np.abs(got[:, :2] - want[:, :2])) < 1e-12
        if tail is not None:
            assert np.all(np.any(got[-tail:] != poses[-tail:], axis=1))
    args = (1.25, -3.5, 3.0, 0.3, 0.2, 0.5)
    for noise, kw in ((z, {}), (z_dev, dict(seed=seed, step=step, first=first))):
        want = O.pf_init(*args, noise)
        got = _init(torch, matcher, n, args, None if kw else noise, **kw)
        assert np.array_equal(got, want)
        if tail is not None:
            assert np.all(got[-tail:] != -1.0e30)


def test_noise_beyond_the_grid_cap(torch, matcher):
    """n = 4096 * 256 + 257: 257 threads go round noise_kernel's loop a second time."""
    seed, step, first = 20240, 3, 11
    z = _noise(torch, matcher, seed, step, first, N_BEYOND).cpu().numpy()
    assert np.all(np.isfinite(z[-300:]))
    ratio = _noise_ratio(z, seed, step, first)
    print("noise ratio beyond the cap: %.3f" % ratio)
    assert ratio <= NOISE_B, ratio


def test_motion_and_init_beyond_the_grid_cap(torch, matcher):
    seed, step, first = 20240, 3, 11
    z_dev = _noise(torch, matcher, seed, step, first, N_BEYOND).cpu().numpy()
    _check_motion_and_init(torch, matcher, N_BEYOND, np.random.default_rng(41), seed, step, first,
                           z_dev, tail=300)


def _check_statistics_fsum(poses, w, out, w_got):
    """updateStatistics from correctly rounded sums (math.fsum of the float64 terms), at the
    tolerances of _check_statistics."""
    th = poses[:, 2]
    S = [math.fsum(t.tolist()) for t in _moment_terms(poses, w)]
    sw = S[0]
    mx, my, mth = S[1] / sw, S[2] / sw, math.atan2(S[4] / sw, S[3] / sw)
    r = np.fmod((mth - th) + math.pi, 2.0 * math.pi)
    d = np.where(r <= 0.0, r + math.pi, r - math.pi)
    var = math.fsum(((w / sw) * d * d).tolist())
    assert np.allclose(w_got, w / sw, rtol=1e-12, atol=0)
    assert np.allclose(out[1:4], [mx, my, mth], rtol=1e-11, atol=1e-13)
    assert np.allclose([out[4], out[5], out[6]],
                       [S[5] / sw - mx * mx, S[6] / sw - mx * my, S[7] / sw - my * my],
                       rtol=1e-8, atol=1e-12)
    assert 0.125 + out[7] == pytest.approx(0.125 + var, rel=1e-11, abs=0)


@pytest.mark.parametrize("uniform", [False, True])
def test_statistics_beyond_the_grid_cap(torch, matcher, uniform):
    """Given weights: against the oracle, and against correctly rounded sums.  Uniform weights:
    against correctly rounded sums only -- the oracle adds the weights one after the other as the
    reference does, and 1,048,833 equal addends 1/n drift by 1.2e-11 of their sum in that loop
    (measured on the CPU against math.fsum; random weights: 2.5e-14), which is the oracle's own
    error and above the 1e-12 the weights are held to."""
    rng = np.random.default_rng(43)
    n = N_BEYOND
    poses = _wrap_poses(rng, n)
    w = np.full(n, 1.0 / n) if uniform else rng.uniform(0.1, 2.0, size=n)
    sums, out, w_got = _statistics(torch, matcher, poses, w, uniform)
    if not uniform:
        _check_statistics(poses, w, out, w_got, tail=300)
    _check_statistics_fsum(poses, w, out, w_got)
    sw = math.fsum(w.tolist())
    assert abs(sums[0] - sw) <= (_moment_depth(n) + 3) * 2.0 ** -53 * sw and out[0] == sums[0]
    assert abs(w_got.sum() - 1.0) < 1e-12
    assert np.allclose(w_got[-300:], w[-300:] / sw, rtol=1e-12, atol=0)       # the tail was written
    if not uniform:
        assert np.all(w_got[-300:] != w[-300:])


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_small_and_ragged_sizes(torch, matcher, n):
    """One particle, a partial wave, whole waves plus one lane, a block whose later waves hold
    no particle, a second block of one lane: wave_sum over idle lanes and the sh[] rows of idle
    waves must add exact zeros."""
    rng = np.random.default_rng(1000 + n)
    seed, step, first = 5 + n, 2, 70000
    z_dev = _noise(torch, matcher, seed, step, first, n).cpu().numpy()
    assert _noise_ratio(z_dev, seed, step, first) <= NOISE_B
    _check_motion_and_init(torch, matcher, n, rng, seed, step, first, z_dev, tail=min(n, 300))
    poses = _wrap_poses(rng, n)
    for uniform in (False, True):
        w = np.full(n, 1.0 / n) if uniform else rng.uniform(0.1, 2.0, size=n)
        _, out, w_got = _statistics(torch, matcher, poses, w, uniform)
        _check_statistics(poses, w, out, w_got, tail=min(n, 300))


@pytest.mark.parametrize("uniform", [False, True])
def test_one_particle_is_its_own_mean(torch, matcher, uniform):
    """n = 1 with a weight that is a power of two (0.25; uniform: 1/n = 1), so every product and
    quotient by it is exact: mean x / y are the pose's bits and the covariance sums
    (w x x) / w - mean_x mean_x are exactly 0.  The circular mean is atan2(sin t, cos t): that is
    t to the bit at t = 0 (then the theta variance increment is exactly 0 too); at another
    heading it is t to the functions' last places -- sincos within 2 ulp moves the angle by at
    most 2^-51, atan2 within 2 ulp by 2^-51 |t| -- and the increment at most that squared."""
    w = np.array([1.0 if uniform else 0.25])
    for pose in ([1.2345678901234567, -7.654321098765432, 0.0],
                 [-3.3333333333333335, 0.1234567890123456, 2.718281828459045]):
        poses = np.array([pose])
        sums, out, w_got = _statistics(torch, matcher, poses, w, uniform)
        _check_statistics(poses, w, out, w_got)
        assert w_got[0] == 1.0 and out[0] == w[0] and sums[0] == w[0]
        assert out[1] == pose[0] and out[2] == pose[1]
        assert out[4] == 0.0 and out[5] == 0.0 and out[6] == 0.0
        tol = 2.0 ** -51 * (1.0 + abs(pose[2]))
        print("n = 1: mean theta - theta = %.3e, variance increment %.3e" % (out[3] - pose[2], out[7]))
        if pose[2] == 0.0:
            assert out[3] == 0.0 and out[7] == 0.0
        else:
            assert abs(out[3] - pose[2]) <= tol and 0.0 <= out[7] <= tol * tol


def _moment_terms(poses, w):
    """The eight terms of every particle in float64, in the kernel's association."""
    x, y, th = poses[:, 0], poses[:, 1], poses[:, 2]
    c, s = np.cos(th), np.sin(th)
    return [w, w * x, w * y, w * c, w * s, (w * x) * x, (w * x) * y, (w * y) * y]


def _moment_depth(n):
    """The most additions a term passes through on its way into a sum, read off moments_kernel
    and moments_reduce_kernel: the thread's own trips round its loop, 6 levels of the 64-lane
    wave sum, 3 adds for the block's four waves, the reducer thread's loop over its blocks and
    the 8 levels of its 256-wide tree."""
    blocks = min(-(-n // BLOCK), CAP_BLOCKS)
    trips = -(-n // (blocks * BLOCK))
    return trips + 6 + 3 + -(-blocks // 256) + 8


@pytest.mark.parametrize("weights", ["plain", "zeros", "span", "uniform"])
@pytest.mark.parametrize("n", [257, 70001, N_BEYOND])
def test_moment_sums_against_fsum(torch, matcher, n, weights):
    """The eight raw sums of pose_moments_launch against math.fsum (the correctly rounded sum) of
    the same float64 terms.  Bound: every addition rounds by at most 2^-53 of a partial sum, which
    is at most sum |term|, and a term meets _moment_depth(n) = D of them; its two products and the
    last ulps of the device's sincos against numpy's are 3 2^-53 |term| more:
        |sum_dev - fsum| <= (D + 3) 2^-53 sum |term|.
    Largest |sum_dev - fsum| / bound observed on an MI355X: 0.14 (n = 257, D = 19); 0.05 at
    n = 1,048,833 (D = 35)."""
    rng = np.random.default_rng(n + 7)
    poses = _wrap_poses(rng, n)
    if weights == "zeros":
        w = rng.uniform(0.1, 2.0, size=n) * (rng.random(n) < 0.5)
    elif weights == "span":
        w = 10.0 ** rng.uniform(-12.0, 0.0, size=n)
        w[0], w[-1] = 1.0e-12, 1.0
    elif weights == "uniform":
        w = np.full(n, 1.0 / n)
    else:
        w = rng.uniform(0.1, 2.0, size=n)
    sums, _, _ = _statistics(torch, matcher, poses, w, weights == "uniform")
    depth = _moment_depth(n)
    worst = 0.0
    for k, term in enumerate(_moment_terms(poses, w)):
        exact = math.fsum(term.tolist())
        bound = (depth + 3) * 2.0 ** -53 * math.fsum(np.abs(term).tolist())
        worst = max(worst, abs(sums[k] - exact) / bound)
        assert abs(sums[k] - exact) <= bound, (k, sums[k], exact, bound)
    print("moment sums n=%d %s: D=%d, worst |err| / bound = %.3f" % (n, weights, depth, worst))


# ---- designed values at the angle wraps --------------------------------------------------------

def _normalize_angle(a):
    """angles::normalize_angle on Python floats; math.fmod is exact, as the device's is."""
    r = math.fmod(a + math.pi, 2.0 * math.pi)
    return r + math.pi if r <= 0.0 else r - math.pi


ZERO_ALPHAS = [0.0, 0.0, 0.0, 0.0, 0.0]
THREE_PI = 3.0 * math.pi
# (heading, dth) of a pure rotation: trans = 0, rot1 = 0, rot2 = normalize_angle(dth) held as float.
# 1.5 is a float, and pi - 1.5, 3 pi - 1.5 are exact double differences, so the sums land where named.
WRAP_CASES = [
    (math.pi - 1.5, 1.5), (-(math.pi - 1.5), -1.5),         # exactly +pi, exactly -pi
    (math.pi, 0.0), (-math.pi, 0.0),
    (-1.5, 1.5), (1.5, -1.5), (0.0, 0.0),                   # exactly 0
    (THREE_PI - 1.5, 1.5), (-(THREE_PI - 1.5), -1.5),       # 3 pi, -3 pi
    (THREE_PI, 0.0), (-THREE_PI, 0.0),
    (1.0e6 + 0.25, 1.5), (-1.0e6 - 0.25, -1.5), (1.0e6 + 0.25, -1.5),
    (3.0, 0.25), (-3.0, -0.25),                             # across the wrap, off the lattice
]


@pytest.mark.parametrize("given_noise", [True, False])
def test_motion_lands_on_the_designed_wraps(torch, matcher, given_noise):
    """All alphas zero: every sigma is 0 and the draw is its mean whatever the noise.  The new
    heading is normalize_angle((theta + float(rot1)) + float(rot2)) in exact double arithmetic
    (two adds and an exact fmod), so Python's math.fmod on the same doubles has the same bits."""
    rng = np.random.default_rng(5)
    for dth in sorted({d for _, d in WRAP_CASES}):
        heads = [t for t, d in WRAP_CASES if d == dth]
        poses = np.array([[0.5 * i - 1.0, 2.0 - 0.25 * i, t] for i, t in enumerate(heads)])
        z = rng.standard_normal((len(poses), 3)).astype(np.float32) if given_noise else None
        got = _motion(torch, matcher, poses, (0.0, 0.0, dth), ZERO_ALPHAS, z, 12, 34, 56)
        rot2 = float(np.float32(_normalize_angle(dth - 0.0)))
        want = [_normalize_angle((t + 0.0) + rot2) for t in heads]
        assert got[:, 2].tolist() == want, (dth, got[:, 2].tolist(), want)
        assert np.array_equal(got[:, :2], poses[:, :2])          # t = 0: x + 0 * cos
        oracle, _ = O.motion_sample(0.0, 0.0, dth, ZERO_ALPHAS, poses,
                                    np.zeros((len(poses), 3), dtype=np.float32))
        assert np.array_equal(got, oracle)
        for t, th in zip(heads, got[:, 2]):
            if abs(t + rot2) == math.pi:
                assert th == math.pi                             # -pi comes out +pi: the <= 0 branch
            if t + rot2 == 0.0:
                assert th == 0.0
    # the designed sums are what their names say
    assert (math.pi - 1.5) + 1.5 == math.pi and (THREE_PI - 1.5) + 1.5 == THREE_PI
    assert _normalize_angle(THREE_PI) == math.pi and _normalize_angle(-THREE_PI) == math.pi


@pytest.mark.parametrize("given_noise", [True, False])
def test_init_at_plus_and_minus_pi(torch, matcher, given_noise):
    """theta = +-pi is held as float (3.14159274 > pi), sigma 0: float pi wraps to just above
    -pi, float -pi to just below +pi."""
    n = 65
    z = np.random.default_rng(6).standard_normal((n, 3)).astype(np.float32) if given_noise else None
    for theta in (math.pi, -math.pi, 3.0 * math.pi, 0.0):
        got = _init(torch, matcher, n, (0.5, -0.25, theta, 0.0, 0.0, 0.0), z, 12, 34, 56)
        want = _normalize_angle(float(np.float32(theta)))
        assert np.all(got[:, 0] == 0.5) and np.all(got[:, 1] == -0.25)
        assert got[:, 2].tolist() == [want] * n
        assert np.array_equal(got, O.pf_init(0.5, -0.25, theta, 0.0, 0.0, 0.0,
                                             np.zeros((n, 3), dtype=np.float32)))
    assert _normalize_angle(float(np.float32(math.pi))) < -3.14159
    assert _normalize_angle(float(np.float32(-math.pi))) > 3.14159


def test_circular_mean_at_pi(torch, matcher):
    """Two particles at headings +3.0 and -3.0.  Equal weights: the sines cancel to +0, the cosine
    sum is negative, atan2(+0, < 0) is pi exactly; each angular distance is pi - 3 through exact
    adds and an exact fmod, so the theta variance increment is (pi - 3)^2.  Weights 3 : 1: the oracle."""
    poses = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, -3.0]])
    for uniform, w in ((False, [1.0, 1.0]), (True, [0.5, 0.5]), (False, [0.7, 0.7])):
        w = np.array(w)
        sums, out, w_got = _statistics(torch, matcher, poses, w, uniform)
        assert sums[4] == 0.0 and sums[3] < 0.0
        assert out[3] == math.pi
        assert out[7] == pytest.approx((math.pi - 3.0) ** 2, rel=1e-15, abs=0)
        assert w_got.tolist() == [0.5, 0.5]
        _check_statistics(poses, w, out, w_got)
    w = np.array([3.0, 1.0])
    _, out, w_got = _statistics(torch, matcher, poses, w, False)
    _check_statistics(poses, w, out, w_got)
    _, mean_want, _ = O.pf_update_statistics(poses, w)
    assert 3.0 < mean_want[2] < math.pi and out[3] == pytest.approx(mean_want[2], rel=1e-14, abs=0)
    w = np.array([1.0, 3.0])
    _, out, w_got = _statistics(torch, matcher, poses, w, False)
    _check_statistics(poses, w, out, w_got)
    assert -math.pi < out[3] < -3.0
