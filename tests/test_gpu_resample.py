"""ParticleFilter::resample on the device (csrc/resample/ndt2d_resample.hip) against the host form.

Every comparison is against `kld_resample_native` (ndt2d_kld_resample, the host loop) and, on
small cases, a plain Python transcription of the reference loop (src/particle_filter.cpp:94-134)
-- never against the device code itself -- and every comparison is np.array_equal on the bits: no
tolerance, no excluded case.

Timing (test_resample_times, an MI355X, stream-synchronised wall time of ParticleFilter.resample,
median of 20 after 5 warm-ups): see profiles/resample_timing.json for the recorded figures."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from ndt_2d_amd import ScanMatcherNDT, _capi, synth
from ndt_2d_amd.particle_filter import KD_LEAF, MotionModel, ParticleFilter, kld_resample_native
from noise_restatement import philox4x32_10

pytestmark = pytest.mark.gpu

N_CAP = 100000
MAX_CAP = 1 << 18
SIZES = (1, 2, 63, 64, 65, 500, 4097, 100000)
SEEDS_PER_SIZE = 26           # 8 sizes x 26 = 208 random sets
KLD = ((0.01, 2.3), (0.05, 1.0), (0.002, 3.0))   # the node's, and two others


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    """(matcher, stream, resampler): one resampler for the whole module, so that every case
    also runs on a workspace that other sizes have used before it."""
    m = ScanMatcherNDT(0)
    m.initialize("resample", **synth.matcher_params(1))
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    r = m.create_resampler(N_CAP, MAX_CAP)
    yield m, s, r
    r.close()


# ---- the references ------------------------------------------------------------------------

def py_key(value, leaf):
    q = np.float64(value) / np.float64(leaf)
    if q >= 2147483647.0:
        return 2147483647
    if q <= -2147483648.0:
        return -2147483648
    return int(q) if q == q else 0


def py_reference_loop(particles, weights, min_particles, max_particles, kld_err, kld_z, uniforms,
                      leaf=KD_LEAF):
    """ParticleFilter::resample's loop transcribed (particle_filter.cpp:94-134): a running cdf,
    libstdc++'s upper_bound, a set of leaf keys, Mx after every insert."""
    with np.errstate(all="ignore"):
        n = len(weights)
        cdf = np.empty(n)
        total = np.float64(0.0)
        for i in range(n):
            total = total + np.float64(weights[i])
            cdf[i] = total
        out = []
        if max_particles == 0:
            return np.zeros(0, dtype=np.uint32)
        leaves = set()
        mx = max_particles
        while len(out) < max(min_particles, mx):
            val = np.float64(uniforms[len(out)]) * total
            first, length = 0, n
            while length > 0:
                half = length >> 1
                if val < cdf[first + half]:
                    length = half
                else:
                    first += half + 1
                    length -= half + 1
            p = min(first, n - 1)
            leaves.add(tuple(py_key(particles[p][d], leaf[d]) for d in range(3)))
            out.append(p)
            k = len(leaves)
            if k > 1:
                a = np.float64(k - 1) / (np.float64(2.0) * np.float64(kld_err))
                b = np.float64(2.0) / (np.float64(9.0) * np.float64(k - 1))
                c = np.float64(1.0) - b + np.sqrt(b) * np.float64(kld_z)
                m = a * c * c * c
                mx = (1 << 64) - 1 if m >= 1.8446744073709552e19 else (int(m) if m > 0.0 else 0)
            if len(out) >= max_particles:
                break
        return np.array(out, dtype=np.uint32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the device side -----------------------------------------------------------------------

def device_resample(torch, ctx, particles, weights, min_p, max_p, kld_err, kld_z, uniforms,
                    leaf=KD_LEAF, resampler=None, seed=0, step=0):
    """(indices, particles_out, weights_out) of the count kept, all through device pointers."""
    m, s, r = ctx
    r = resampler or r
    cap = max(int(max_p), 1)
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(np.ascontiguousarray(particles, dtype=np.float64).reshape(-1, 3)).cuda()
        d_w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).cuda()
        d_u = None if uniforms is None else torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64)).cuda()
        o_p = torch.full((cap, 3), -7.0, dtype=torch.float64, device="cuda")
        o_w = torch.full((cap,), -7.0, dtype=torch.float64, device="cuda")
        o_i = torch.full((cap,), 0x7fffffff, dtype=torch.int32, device="cuda")
        r.launch(d_p.data_ptr(), d_w.data_ptr(), len(d_w), min_p, max_p, kld_err, kld_z,
                 o_p.data_ptr(), o_w.data_ptr(), o_i.data_ptr(),
                 None if d_u is None else d_u.data_ptr(), seed, step, leaf)
        count = r.fetch()
        assert 0 <= count <= max_p
        # nothing behind the count is written
        assert bool((o_w[count:] == -7.0).all()) and bool((o_i[count:] == 0x7fffffff).all())
        idx = o_i[:count].cpu().numpy().view(np.uint32)
        return idx, o_p[:count].cpu().numpy(), o_w[:count].cpu().numpy()


def device_statistics(torch, ctx, particles, weights):
    """pose_moments + pf_finalize on a set: (normalised weights, the 16 stats doubles)."""
    m, s, _ = ctx
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(np.ascontiguousarray(particles)).cuda()
        d_w = torch.from_numpy(np.ascontiguousarray(weights)).cuda()
        st = torch.zeros(_capi.POSE_STATS_DOUBLES + _capi.PF_RESULT_DOUBLES, dtype=torch.float64,
                         device="cuda")
        m.pose_moments_launch(d_p.data_ptr(), len(d_w), d_w.data_ptr(), st.data_ptr())
        m.pf_finalize_launch(d_p.data_ptr(), len(d_w), d_w.data_ptr(), st.data_ptr(),
                             st.data_ptr() + 8 * _capi.POSE_STATS_DOUBLES)
        m.synchronize()
        return d_w.cpu().numpy(), st.cpu().numpy()


def check_case(torch, ctx, particles, weights, min_p, max_p, kld_err, kld_z, uniforms, leaf=KD_LEAF,
               python_too=False, statistics=False, resampler=None):
    want = kld_resample_native(particles, weights, min_p, max_p, kld_err, kld_z, uniforms, leaf)
    if python_too:
        ref = py_reference_loop(particles, weights, min_p, max_p, kld_err, kld_z, uniforms, leaf)
        assert np.array_equal(ref, want)
    idx, got_p, got_w = device_resample(torch, ctx, particles, weights, min_p, max_p, kld_err, kld_z,
                                        uniforms, leaf, resampler)
    tag = (len(weights), min_p, max_p, kld_err, kld_z, len(want), len(idx))
    assert len(idx) == len(want), tag
    assert np.array_equal(idx, want), tag
    pa = np.ascontiguousarray(particles, dtype=np.float64).reshape(-1, 3)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    assert same_bits(got_p, pa[want]), tag
    assert same_bits(got_w, w[want]), tag
    if statistics and len(want) > 0:
        w_dev, st_dev = device_statistics(torch, ctx, got_p, got_w)
        w_ref, st_ref = device_statistics(torch, ctx, pa[want], w[want])
        assert same_bits(w_dev, w_ref) and same_bits(st_dev, st_ref), tag
    return want


# ---- random sets ---------------------------------------------------------------------------

WEIGHT_KINDS = ("uniform", "measure-like", "mostly-zero", "dominant", "unnormalised")
STOP_KINDS = ("min", "mx", "max", "max<min", "max==0")


def random_case(n, seed):
    """A particle set, weights, (min, max), (kld_err, kld_z), uniforms.  The spread of the poses and
    the (min, max) pair are chosen for the stop rule named by STOP_KINDS[(seed // 5) % 5]."""
    rng = np.random.default_rng(1000003 * n + seed)
    wk = WEIGHT_KINDS[seed % 5]
    sk = STOP_KINDS[(seed // 5) % 5]
    kld_err, kld_z = KLD[seed % 3]
    if sk == "min":          # a tight cluster: few leaves, Mx small, min decides
        sigma, min_p, max_p = 0.2, max(n, 8), 2 * max(n, 8) + 3
    elif sk == "mx":         # a room-sized cloud: Mx lands between a small min and a large max
        sigma, min_p, max_p = 1.5, 3, min(2 * N_CAP, max(40 * n, 4000))
    elif sk == "max":        # every draw a leaf of its own: Mx outgrows max
        sigma, min_p, max_p = 400.0, 2, max(n // 2, 5)
    elif sk == "max<min":
        sigma, min_p, max_p = 1.5, n + 10, max(n // 3, 1)
    else:
        sigma, min_p, max_p = 1.5, 5, 0
    p = rng.normal(0.0, sigma, size=(n, 3))
    p[:, 2] = rng.uniform(-np.pi, np.pi, size=n) if sigma > 1.0 else rng.normal(0.0, 0.05, size=n)
    if wk == "uniform":
        w = np.full(n, 1.0 / n)
    elif wk == "measure-like":       # raw likelihood sums over 300 orders of magnitude
        w = 10.0 ** rng.uniform(-300.0, 0.0, size=n)
    elif wk == "mostly-zero":
        w = rng.uniform(0.0, 1.0, size=n) * (rng.uniform(size=n) < 0.1)
        w[rng.integers(n)] = 0.5     # (never all zero)
    elif wk == "dominant":
        w = rng.uniform(0.0, 1e-6, size=n)
        w[rng.integers(n)] = 1.0
    else:
        w = rng.uniform(0.0, 1e6, size=n)
    u = rng.random(max(max_p, 1))
    return p, w, min_p, max_p, kld_err, kld_z, u, sk


SCAN_N = 1200                 # leaves of scan_case
SCAN_MAX = 65536 + 256 + 1    # 258 tiles of 256 draws: two a thread of the scan, the last one ragged


def scan_case():
    """A stop that only the inclusive rank of a late draw decides: 1,200 particles, each in a leaf of
    its own, so that after the first few thousand draws every draw has k = 1,200 leaves before it
    and Mx(1,200) = 65,724 for (0.01, 2.3).  The host loop keeps 65,724 draws: beyond the scan's
    first chunk of tiles and beyond draw 65,536, inside the last whole tile, below max."""
    rng = np.random.default_rng(SCAN_N)
    p = np.zeros((SCAN_N, 3))
    p[:, 0] = (np.arange(SCAN_N) % 40 + 0.5) * KD_LEAF[0]
    p[:, 1] = (np.arange(SCAN_N) // 40 + 0.5) * KD_LEAF[1]
    p[:, 2] = rng.uniform(-0.1, 0.1, size=SCAN_N)
    return p, rng.uniform(0.5, 1.0, size=SCAN_N), 3, SCAN_MAX, 0.01, 2.3, rng.random(SCAN_MAX)


@pytest.mark.parametrize("n", SIZES + (pytest.param(None, id="scan-two-tiles-a-thread"),))
def test_random_sets_match_the_host_loop(torch, ctx, n):
    if n is None:          # the designed set of scan_case, not a size of random sets
        want = check_case(torch, ctx, *scan_case(), statistics=True)
        assert len(want) == 65724 and len(set(want.tolist())) == SCAN_N
        return
    ended = set()
    for seed in range(SEEDS_PER_SIZE):
        p, w, min_p, max_p, kld_err, kld_z, u, sk = random_case(n, seed)
        want = check_case(torch, ctx, p, w, min_p, max_p, kld_err, kld_z, u,
                          python_too=(n <= 500), statistics=True)
        c = len(want)
        if max_p == 0:
            ended.add("max==0")
            assert c == 0
        elif max_p < min_p:
            ended.add("max<min")
            assert c == max_p
        elif c == max_p:
            ended.add("max")
        elif c == min_p:
            ended.add("min")
        else:
            assert min_p < c < max_p
            ended.add("mx")
    # (what ended each loop is a property of the host form: tests/test_particle_host.py-style
    # CPU arithmetic; from 500 particles on every rule occurs)
    if n >= 500:
        assert ended == set(STOP_KINDS), ended


# ---- designed draws ------------------------------------------------------------------------

def test_draws_on_and_beside_cdf_entries(torch, ctx):
    """u * total exactly on a cdf entry and on its two neighbouring doubles; u = 0 in front of
    leading zero weights; u = nextafter(1, 0) (the clamp)."""
    n = 64
    rng = np.random.default_rng(4)
    w = np.zeros(n)
    w[3:63] = rng.integers(1, 100, size=60) / 1024.0    # dyadic: every partial sum is exact
    w[10] = 0.0                                          # a repeated cdf entry in the middle
    w[63] = 8.0 - w[:63].sum()                           # total = 8: u = c / 8 and u * 8 are exact
    cdf = np.cumsum(w)
    total = cdf[-1]
    assert total == 8.0
    us = [0.0, np.nextafter(1.0, 0.0)]
    for c in cdf[2:40]:
        u = c / total
        for v in (np.nextafter(u, 0.0), u, np.nextafter(u, 1.0)):
            if 0.0 <= v < 1.0:
                us.append(v)
    hit = sum(1 for u in us if (u * total) in cdf)
    assert hit >= 30                          # the designed uniforms do land on entries
    us = np.array(us)
    p = np.random.default_rng(5).normal(0.0, 30.0, size=(n, 3))
    want = check_case(torch, ctx, p, w, len(us), len(us), 0.01, 2.3, us, python_too=True)
    assert want[0] == 3                       # u = 0 skips the leading zero weights
    assert want[1] == n - 1


def test_unsorted_cdf_negative_and_nan_weight(torch, ctx):
    """A negative weight and a NaN weight in the middle: the cdf is not sorted, and only the same
    bisection gives the same answer."""
    rng = np.random.default_rng(11)
    for n in (65, 500, 4097):
        p = rng.normal(0.0, 5.0, size=(n, 3))
        for bad in ("negative", "nan", "both"):
            w = rng.uniform(0.1, 1.0, size=n)
            if bad in ("negative", "both"):
                w[n // 3] = -0.4 * w[: n // 3].sum()
            if bad in ("nan", "both"):
                w[n // 2] = np.nan
            u = rng.random(2 * n)
            want = check_case(torch, ctx, p, w, n, 2 * n, 0.01, 2.3, u, python_too=(n <= 500))
            assert len(want) >= n
            if bad != "negative":
                assert (want == n - 1).all()   # total is NaN: every comparison fails, the clamp holds


# ---- designed keys -------------------------------------------------------------------------

def test_key_truncates_toward_zero_and_pins(torch, ctx):
    leaf = KD_LEAF
    # +-0.3 / 0.5 -> 0: one leaf; k stays 1 and the loop runs to max_particles
    p = np.array([[0.3, 0.3, 0.1], [-0.3, -0.3, -0.1], [0.3, -0.3, 0.1], [-0.3, 0.3, -0.1]])
    w = np.full(4, 0.25)
    u = np.random.default_rng(1).random(300)
    want = check_case(torch, ctx, p, w, 5, 300, 0.01, 2.3, u, python_too=True)
    assert len(want) == 300 and len(set(want.tolist())) == 4
    # 1e300, -1e300 and a NaN theta pin to +-2^31 and 0
    p = np.array([[1e300, 0.0, 0.0], [-1e300, 0.0, 0.0], [0.0, 0.0, np.nan], [0.0, 0.0, 0.0],
                  [np.inf, -np.inf, 0.0], [2147483647.0 * 0.5, 0.0, 0.0], [1e300, 0.0, 0.0]])
    w = np.full(len(p), 1.0)
    u = np.random.default_rng(2).random(400)
    for max_p in (7, 60, 400):
        check_case(torch, ctx, p, w, 3, max_p, 0.01, 2.3, u, python_too=True)
    # keys that differ in one component only
    base = np.array([3.2, -7.9, 1.0])
    rows = [base]
    for d in range(3):
        for step in (1, 2, -1):
            r = base.copy()
            r[d] += step * leaf[d]
            rows.append(r)
    p = np.array(rows)
    w = np.full(len(p), 1.0)
    u = np.random.default_rng(3).random(2000)
    want = check_case(torch, ctx, p, w, 2, 2000, 0.01, 2.3, u, python_too=True)
    assert 2 < len(want) < 2000               # ten leaves: Mx ends it


def test_one_leaf_and_all_distinct_leaves_at_100000(torch, ctx):
    rng = np.random.default_rng(21)
    n = 100000
    # one leaf
    p = rng.uniform(0.01, 0.19, size=(n, 3))
    w = rng.uniform(0.5, 1.5, size=n)
    u = rng.random(n)
    want = check_case(torch, ctx, p, w, 10, n, 0.01, 2.3, u, statistics=True)
    assert len(want) == n
    # max_particles distinct leaves: particle j sits alone in leaf (j, 0, 0); the weights make draw
    # i pick particle perm[i], so every draw is a new key and the table fills to max / size
    p = np.zeros((n, 3))
    p[:, 0] = (np.arange(n) + 0.5) * 0.5
    w = np.full(n, 1.0)
    perm = rng.permutation(n)
    u = (perm + 0.5) / n
    want = check_case(torch, ctx, p, w, n, n, 0.01, 2.3, u)
    assert np.array_equal(want, perm.astype(np.uint32))


def test_keys_congruent_modulo_the_table_size(torch, ctx):
    """The table hashes a key (kx, ky, kz) to slot
        (kx * 0x9E3779B1 + ky * 0x85EBCA77 + kz * 0xC2B2AE3D) mod T,
    T = the power of two >= max(64, 2 * max_particles), and probes linearly.  Keys whose components
    differ by multiples of T therefore all start at one slot: with max_particles = 100, T = 256,
    the particles below sit in leaves kx = 256 j (and ky = 256 j), one probe chain of 100."""
    max_p = 100
    t = 256
    n = 100
    p = np.zeros((n, 3))
    p[:50, 0] = (np.arange(50) * t + 0.5) * KD_LEAF[0]
    p[50:, 1] = ((np.arange(50) + 1) * t + 0.5) * KD_LEAF[1]
    from ndt_2d_amd.particle_filter import kld_leaf_keys
    keys = kld_leaf_keys(p)
    h = (keys[:, 0] * 0x9E3779B1 + keys[:, 1] * 0x85EBCA77 + keys[:, 2] * 0xC2B2AE3D) % t
    assert len(set(h.tolist())) == 1 and len(np.unique(keys, axis=0)) == n
    rng = np.random.default_rng(8)
    w = np.full(n, 1.0)
    for trial in range(4):
        u = rng.random(max_p)
        want = check_case(torch, ctx, p, w, max_p, max_p, 0.01, 2.3, u, python_too=True)
        assert len(want) == max_p
    # and with Mx deciding (few draws, each a new congruent key)
    want = check_case(torch, ctx, p, w, 2, max_p, 0.5, 0.1, rng.random(max_p), python_too=True)
    assert len(want) < max_p


# ---- determinism and reuse -----------------------------------------------------------------

def test_repeats_are_identical_and_the_table_is_cleared(torch, ctx):
    big = random_case(100000, 6)      # stop by Mx, many leaves
    small = random_case(63, 11)
    out_big = [device_resample(torch, ctx, *big[:7]) for _ in range(3)]
    for o in out_big[1:]:
        assert all(same_bits(a, b) for a, b in zip(o, out_big[0]))
    # a small set right after the large one, and the large one again
    check_case(torch, ctx, *small[:7], python_too=True)
    check_case(torch, ctx, *big[:7])
    check_case(torch, ctx, *small[:7], python_too=True)


# ---- the Philox stream ---------------------------------------------------------------------

def philox_uniforms(seed, step, first, n):
    i = np.uint64(first) + np.arange(n, dtype=np.uint64)
    m32 = np.uint64(0xffffffff)
    ctr = np.stack([i & m32, i >> np.uint64(32), np.full(n, step & 0xffffffff, dtype=np.uint64),
                    np.full(n, step >> 32, dtype=np.uint64)], axis=-1)
    key = np.stack([np.full(n, seed & 0xffffffff, dtype=np.uint64),
                    np.full(n, seed >> 32, dtype=np.uint64)], axis=-1)
    w = philox4x32_10(ctr, key)
    b = ((w[:, 0] >> np.uint64(5)) << np.uint64(26)) + (w[:, 1] >> np.uint64(6))
    return b.astype(np.float64) * 2.0 ** -53


def test_philox_restatement_known_answers():
    """The published Random123 known answers anchor the restatement the device is held to."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        got = philox4x32_10(np.array([ctr], dtype=np.uint64), np.array([key], dtype=np.uint64))[0]
        assert [int(v) for v in got] == list(out)


def device_uniforms(torch, ctx, seed, step, first, n):
    m, s, r = ctx
    with torch.cuda.stream(s):
        d = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        r.uniforms_launch(seed, step, first, n, d.data_ptr())
        m.synchronize()
        return d.cpu().numpy()


def test_uniform_stream_is_the_philox_restatement(torch, ctx):
    seed, step = 0xC0FFEE1234567, (5 << 32) + 9
    n = 20001
    whole = device_uniforms(torch, ctx, seed, step, 0, n)
    assert same_bits(whole, philox_uniforms(seed, step, 0, n))
    assert (whole >= 0.0).all() and (whole < 1.0).all()
    assert np.array_equal(whole * 2.0 ** 53, np.floor(whole * 2.0 ** 53))   # the 2^-53 grid
    assert abs(whole.mean() - 0.5) < 5.0 / np.sqrt(12.0 * n)
    # a sub-range launch is the slice; 64-bit indices are honoured
    part = device_uniforms(torch, ctx, seed, step, 4097, 1000)
    assert same_bits(part, whole[4097:5097])
    far = device_uniforms(torch, ctx, seed, step, (1 << 40) + 3, 64)
    assert same_bits(far, philox_uniforms(seed, step, (1 << 40) + 3, 64))
    assert not same_bits(device_uniforms(torch, ctx, seed + 1, step, 0, 64), whole[:64])


def test_null_uniforms_draw_the_published_stream(torch, ctx):
    seed, step = 77, 12
    for n, case_seed in ((500, 6), (4097, 7), (100000, 6)):
        p, w, min_p, max_p, kld_err, kld_z, _, _ = random_case(n, case_seed)
        stream = device_uniforms(torch, ctx, seed, step, 0, max_p)
        want = kld_resample_native(p, w, min_p, max_p, kld_err, kld_z, stream)
        a = device_resample(torch, ctx, p, w, min_p, max_p, kld_err, kld_z, None, seed=seed, step=step)
        b = device_resample(torch, ctx, p, w, min_p, max_p, kld_err, kld_z, stream)
        assert np.array_equal(a[0], want)
        assert all(same_bits(x, y) for x, y in zip(a, b))
        other = device_resample(torch, ctx, p, w, min_p, max_p, kld_err, kld_z, None, seed=seed, step=step + 1)
        assert not np.array_equal(other[0][:64], a[0][:64])


# ---- the host-pointer entry point and refusals ---------------------------------------------

def test_host_pointer_entry_matches(ctx):
    m, _, _ = ctx
    for n, seed in ((1, 0), (65, 6), (500, 7), (4097, 12), (4097, 21)):
        p, w, min_p, max_p, kld_err, kld_z, u, _ = random_case(n, seed)
        want = kld_resample_native(p, w, min_p, max_p, kld_err, kld_z, u)
        got = m.pf_resample(p, w, min_p, max_p, kld_err, kld_z, u)
        assert np.array_equal(got, want)


def test_refusals_match_the_host_and_leave_everything_usable(torch, ctx):
    m, s, r = ctx
    L = _capi.lib()
    h = m.device_handle
    n = 100
    p = np.random.default_rng(0).normal(size=(n, 3))
    w = np.full(n, 1.0)
    u = np.random.default_rng(1).random(200)
    lf = np.array(KD_LEAF)
    idx = np.zeros(200, dtype=np.uint32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_uint32))
    cnt = C.c_size_t(99)
    dp = _capi.dptr

    def both(*args):
        host = L.ndt2d_kld_resample(*args)
        dev = L.ndt2d_pf_resample(h, *args)
        assert host == dev, (host, dev)
        return dev

    ok = (dp(p), dp(w), n, 10, 200, 0.01, 2.3, dp(lf), dp(u), 200, ip, C.byref(cnt))
    assert both(*ok) == _capi.OK and cnt.value > 0
    assert both(dp(p), dp(w), n, 10, 200, 0.01, 2.3, dp(lf), dp(u), 200, ip, None) == _capi.ERR_INVALID
    assert both(None, dp(w), n, 10, 200, 0.01, 2.3, dp(lf), dp(u), 200, ip, C.byref(cnt)) == _capi.ERR_INVALID
    assert both(dp(p), None, n, 10, 200, 0.01, 2.3, dp(lf), dp(u), 200, ip, C.byref(cnt)) == _capi.ERR_INVALID
    assert both(dp(p), dp(w), 0, 10, 200, 0.01, 2.3, dp(lf), dp(u), 200, ip, C.byref(cnt)) == _capi.ERR_INVALID
    assert both(dp(p), dp(w), 1 << 32, 10, 200, 0.01, 2.3, dp(lf), dp(u), 200, ip, C.byref(cnt)) == _capi.ERR_INVALID
    assert both(dp(p), dp(w), n, 10, 200, 0.01, 2.3, None, dp(u), 200, ip, C.byref(cnt)) == _capi.ERR_INVALID
    assert both(dp(p), dp(w), n, 10, 200, 0.01, 2.3, dp(lf), None, 200, ip, C.byref(cnt)) == _capi.ERR_INVALID
    assert both(dp(p), dp(w), n, 10, 200, 0.01, 2.3, dp(lf), dp(u), 199, ip, C.byref(cnt)) == _capi.ERR_INVALID
    assert both(dp(p), dp(w), n, 10, 200, 0.01, 2.3, dp(lf), dp(u), 200, None, C.byref(cnt)) == _capi.ERR_INVALID
    cnt.value = 99
    assert both(None, None, 0, 10, 0, 0.01, 2.3, None, None, 0, None, C.byref(cnt)) == _capi.OK   # max == 0 first
    assert cnt.value == 0
    assert L.ndt2d_pf_resample(None, *ok) == _capi.ERR_INVALID

    # the resampler's own: creation, capacities, null pointers, fetch without a launch
    out = C.c_void_p()
    assert L.ndt2d_resampler_create(None, 10, 10, C.byref(out)) == _capi.ERR_INVALID
    assert L.ndt2d_resampler_create(h, 0, 10, C.byref(out)) == _capi.ERR_INVALID
    assert L.ndt2d_resampler_create(h, 1 << 32, 10, C.byref(out)) == _capi.ERR_INVALID
    assert L.ndt2d_resampler_create(h, 10, 10, None) == _capi.ERR_INVALID
    assert L.ndt2d_resampler_destroy(None) == _capi.ERR_INVALID
    small = m.create_resampler(64, 32)
    with torch.cuda.stream(s):
        d_p = torch.from_numpy(p).cuda()
        d_w = torch.from_numpy(w).cuda()
        o_p = torch.zeros((200, 3), dtype=torch.float64, device="cuda")
        o_w = torch.zeros((200,), dtype=torch.float64, device="cuda")
    s.synchronize()
    sr = small._r
    args = dict(n=64, max_p=32)

    def launch(res, particles, weights, n_, max_, leaf, op, ow):
        return L.ndt2d_resample_launch(res, particles, weights, n_, 5, max_, 0.01, 2.3, leaf, None, 1, 2,
                                       op, ow, None)

    good = (d_p.data_ptr(), d_w.data_ptr(), args["n"], args["max_p"], dp(lf), o_p.data_ptr(), o_w.data_ptr())
    assert L.ndt2d_resample_fetch(sr, C.byref(cnt)) == _capi.ERR_STATE
    assert launch(None, *good) == _capi.ERR_INVALID
    assert launch(sr, d_p.data_ptr(), d_w.data_ptr(), 65, 32, dp(lf), o_p.data_ptr(), o_w.data_ptr()) == _capi.ERR_INVALID
    assert b"capacity" in L.ndt2d_resampler_last_error(sr)
    assert launch(sr, d_p.data_ptr(), d_w.data_ptr(), 64, 33, dp(lf), o_p.data_ptr(), o_w.data_ptr()) == _capi.ERR_INVALID
    assert launch(sr, None, d_w.data_ptr(), 64, 32, dp(lf), o_p.data_ptr(), o_w.data_ptr()) == _capi.ERR_INVALID
    assert launch(sr, d_p.data_ptr(), None, 64, 32, dp(lf), o_p.data_ptr(), o_w.data_ptr()) == _capi.ERR_INVALID
    assert launch(sr, d_p.data_ptr(), d_w.data_ptr(), 0, 32, dp(lf), o_p.data_ptr(), o_w.data_ptr()) == _capi.ERR_INVALID
    assert launch(sr, d_p.data_ptr(), d_w.data_ptr(), 64, 32, None, o_p.data_ptr(), o_w.data_ptr()) == _capi.ERR_INVALID
    assert launch(sr, d_p.data_ptr(), d_w.data_ptr(), 64, 32, dp(lf), None, o_w.data_ptr()) == _capi.ERR_INVALID
    assert launch(sr, d_p.data_ptr(), d_w.data_ptr(), 64, 32, dp(lf), o_p.data_ptr(), None) == _capi.ERR_INVALID
    assert launch(sr, d_p.data_ptr(), d_w.data_ptr(), 64, 32, dp(lf), d_p.data_ptr(), o_w.data_ptr()) == _capi.ERR_INVALID
    assert L.ndt2d_resample_uniforms_launch(sr, 0, 0, 0, 10, None) == _capi.ERR_INVALID
    assert L.ndt2d_resample_uniforms_launch(sr, 0, 0, 0, 0, o_w.data_ptr()) == _capi.ERR_INVALID
    assert L.ndt2d_resample_fetch(sr, None) == _capi.ERR_INVALID
    assert L.ndt2d_resample_fetch(sr, C.byref(cnt)) == _capi.ERR_STATE     # nothing was launched by any of these
    # max_particles == 0: nothing kept, NDT2D_OK
    assert launch(sr, None, None, 0, 0, None, None, None) == _capi.OK
    cnt.value = 99
    assert L.ndt2d_resample_fetch(sr, C.byref(cnt)) == _capi.OK and cnt.value == 0
    # after all that, the resampler and the handle still work
    assert launch(sr, *good) == _capi.OK
    assert L.ndt2d_resample_fetch(sr, C.byref(cnt)) == _capi.OK and 5 <= cnt.value <= 32
    stream = device_uniforms(torch, ctx, 1, 2, 0, 32)
    want = kld_resample_native(p[:64], w[:64], 5, 32, 0.01, 2.3, stream)
    assert cnt.value == len(want)
    assert same_bits(o_p[:cnt.value].cpu().numpy(), p[:64][want])
    small.close()
    check_case(torch, ctx, p, w, 10, 200, 0.01, 2.3, u, python_too=True)


# ---- the filter ----------------------------------------------------------------------------

ALPHAS = [0.1, 0.1, 0.1, 0.1, 0.0]


def _cfg1_matcher():
    m = ScanMatcherNDT(0)
    m.initialize("pf", **synth.matcher_params(1))
    m.addScans(synth.map_scans(1))
    return m


def test_filter_with_device_resampling_is_the_host_run(torch):
    """20 update / measure / resample steps on the cfg-1 world, 100 - 500 particles, the same seed:
    particles, weights, count, mean and covariance are bitwise those of the host-resampled run."""
    guess, pts, _ = synth.query_scan(1)
    filters = {}
    for mode in ("host", "device", "device-philox"):
        filters[mode] = ParticleFilter(100, 500, MotionModel(*ALPHAS), _cfg1_matcher(), seed=4242,
                                       resample_on=mode)
        filters[mode].init(guess[0], guess[1], guess[2], 0.15, 0.15, 0.1)
    assert filters["host"]._resampler is None and filters["device"]._resampler is not None
    rng = np.random.default_rng(9)
    counts = []
    for step in range(20):
        dx, dy, dth = rng.normal(0.0, 0.02, size=3)
        for mode, pf in filters.items():
            pf.update(dx, dy, dth)
            pf.measure(pf._matcher, pts)
            pf.resample(0.01, 2.3)
        a, b, c = filters["host"], filters["device"], filters["device-philox"]
        assert len(a.particles) == len(b.particles), step
        assert same_bits(a.particles.cpu().numpy(), b.particles.cpu().numpy()), step
        assert same_bits(a.weights.cpu().numpy(), b.weights.cpu().numpy()), step
        assert same_bits(a.getMean(), b.getMean()) and same_bits(a.getCovariance(), b.getCovariance()), step
        counts.append(len(a.particles))
        # its own draws: another, equally valid run that never leaves the device
        assert c.particles.is_cuda and c.weights.is_cuda
        assert 100 <= len(c.particles) <= 500
        assert np.isfinite(c.getMean()).all() and np.isfinite(c.getCovariance()).all()
        assert abs(float(c.weights.sum()) - 1.0) < 1e-9
    assert all(100 <= n <= 500 for n in counts)
    with pytest.raises(ValueError):
        ParticleFilter(100, 500, MotionModel(*ALPHAS), filters["host"]._matcher, resample_on="gpu")


# ---- times ---------------------------------------------------------------------------------

def _time_resample(pf, particles, weights, kld, runs=20, warmups=5):
    ms = []
    for k in range(warmups + runs):
        with pf._torch.cuda.stream(pf._stream):
            pf.particles = particles.clone()
            pf.weights = weights.clone()
        pf._stream.synchronize()
        t0 = time.perf_counter()
        pf.resample(*kld)          # ends with updateStatistics, which synchronises the stream
        pf._stream.synchronize()
        t1 = time.perf_counter()
        if k >= warmups:
            ms.append((t1 - t0) * 1e3)
    return float(np.median(ms)), len(pf.particles)


def test_resample_times(torch):
    """Stream-synchronised wall time of ParticleFilter.resample through both paths in ONE session,
    median of 20 after 5 warm-ups, at 500 particles and at cfg-5's 1 000 000 (min = max / 10).
    Asserted: at 1 000 000 the device path is faster than the host path (no margin).  Recorded
    only: the 500-particle pair and the kernel time of the cumulative-weights chain.
    NDT2D_RESAMPLE_TIMING_OUT=<file> writes the record that profiles/resample_timing.json holds."""
    record = {}
    rng = np.random.default_rng(55)
    for n_max in (500, 1000000):
        poses = synth.particles(5, n_max)
        if n_max == 500:
            poses[:, :2] *= 4.0 / 95.0
        w = np.exp(-rng.uniform(0.0, 30.0, size=n_max))
        got = {}
        for mode in ("host", "device", "device-philox"):
            m = ScanMatcherNDT(0)
            m.initialize("pf", **synth.matcher_params(1))
            pf = ParticleFilter(n_max // 10, n_max, MotionModel(*ALPHAS), m, seed=1, resample_on=mode)
            with torch.cuda.stream(pf._stream):
                d_p = torch.from_numpy(poses).to(pf.device)
                d_w = torch.from_numpy(w).to(pf.device)
            if pf._resampler is not None:
                pf._resampler.set_timing(True)
            ms, kept = _time_resample(pf, d_p, d_w, (0.01, 2.3))
            got[mode] = dict(ms=ms, kept=kept)
            if pf._resampler is not None:
                got[mode]["cdf_chain_ms"] = pf._resampler.cdf_ms()
                got[mode]["cdf_chain_ns_per_particle"] = got[mode]["cdf_chain_ms"] * 1e6 / n_max
            m.close()
        assert got["host"]["kept"] == got["device"]["kept"]
        record[str(n_max)] = got
        print("resample n=%d: %s" % (n_max, json.dumps(got)))
    out = os.environ.get("NDT2D_RESAMPLE_TIMING_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(dict(what="ParticleFilter.resample, stream-synchronised wall ms, median of 20 after 5 "
                                "warm-ups; cdf_chain_ms = HIP events around cdf_kernel of the last launch",
                           particles=record), f, indent=1, sort_keys=True)
            f.write("\n")
    big = record["1000000"]
    assert big["device"]["ms"] < big["host"]["ms"], big
