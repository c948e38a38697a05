"""Pose clusters on the device (csrc/cluster/ndt2d_cluster.hip; Clusterer, ParticleFilter.clusters /
estimate) against the restatement (tests/cluster_restatement.py, itself pinned by
tests/test_cluster_restatement.py) -- never against the device code itself.

Exactly equal: every particle's label, the header's integers, each record's label, count and Q, and
the order of the records.  Every double statistic lies within 64 * 2^-53 * sum|terms| of the
restatement's math.fsum value -- the bound of a summation tree of depth <= 40 plus the device's sin
and cos; the restatement supplies sum|terms|.  A record holds sums divided by the cluster's W, so the
bound of a mean or a moment is 64 * 2^-53 * sum|terms| / W.  The mean heading lies within 1e-12 rad
where the resultant is at least 0.1 W.  Two calls on the same input give the same bytes.

The compaction's scan is one block of 256 threads over tiles of 256 particles: up to 65,536
particles a thread holds one tile at most, and 65,792 (that capacity plus one tile) is the first
size at which a thread holds two."""
import numpy as np
import pytest

import cluster_restatement as R
from cluster_cases import BOUND, compare
from ndt_2d_amd import Clusterer, MotionModel, Ndt2dError, OccupancyMap, ParticleFilter, ScanMatcherNDT, _capi, synth

pytestmark = pytest.mark.gpu

BEYOND_ONE_SCAN_TILE = 65536 + 256
MAX_PARTICLES = 100000


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def device():
    m = ScanMatcherNDT(0)
    m.initialize("clusters", **synth.matcher_params(1))
    yield m
    m.close()


@pytest.fixture(scope="module")
def clusterer(device):
    """One clusterer for the whole module, so that every call also runs in buffers that other sizes
    have used before it."""
    c = Clusterer(device, MAX_PARTICLES)
    yield c
    c.close()


def raw_bytes(header, records, labels):
    return (repr(tuple(header)).encode(), b"".join(bytes(r) for r in records), labels.tobytes())


def run(torch, c, poses, weights, cell_x=0.5, cell_y=0.5, n_theta=24, max_clusters=8):
    """One launch and fetch: (header, raw records, labels), after checking that a second call on the
    same input gives the same bytes."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    n = len(poses)
    d_p = torch.from_numpy(poses).cuda() if n else None
    d_w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).cuda() if weights is not None and n else None
    torch.cuda.synchronize()                  # (the clusterer launches on the context's stream, not torch's)
    c.set_bins(cell_x, cell_y, n_theta)
    c.set_max_clusters(max_clusters)
    seen = []
    for _ in range(2):
        c.launch(d_p.data_ptr() if n else None, d_w.data_ptr() if d_w is not None else None, n)
        header, records = c.fetch_raw()
        seen.append((header, records, c.labels()))
    a, b = (raw_bytes(*s) for s in seen)
    assert a[1] == b[1] and a[2] == b[2], "two calls on the same input differ"
    assert seen[0][0]._replace(rounds=0) == seen[1][0]._replace(rounds=0)
    return seen[0]


def blobs(rng, n, centres, sigma=(0.12, 0.12, 0.08), shares=None):
    """n particles round the centres (x, y, theta), and weights that sum to 1."""
    centres = np.asarray(centres, dtype=np.float64)
    which = rng.integers(0, len(centres), size=n) if shares is None else rng.choice(len(centres), size=n, p=shares)
    poses = centres[which] + rng.normal(size=(n, 3)) * np.asarray(sigma)
    w = rng.random(n) + 0.05
    return poses, w / w.sum(), which


def in_bins(rng, n, bin_keys, cell=0.5, n_theta=24):
    """n particles spread evenly inside the bins of the given keys, well off the bins' faces."""
    k = np.asarray(bin_keys, dtype=np.float64)[np.arange(n) % len(bin_keys)]
    u = 0.2 + 0.6 * rng.random((n, 3))
    width = 2.0 * np.pi / n_theta
    return np.stack([(k[:, 0] + u[:, 0]) * cell, (k[:, 1] + u[:, 1]) * cell, -np.pi + (k[:, 2] + u[:, 2]) * width], axis=1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, BEYOND_ONE_SCAN_TILE])
def test_sizes_on_random_blobs(torch, clusterer, n):
    rng = np.random.default_rng(n)
    poses, w, _ = blobs(rng, n, [(-3.2, 1.1, 0.4), (4.3, -2.7, -2.0), (0.2, 0.3, 3.0), (9.1, 9.4, -0.9), (-7.7, 6.0, 1.5)],
                        sigma=(0.3, 0.3, 0.2))
    compare(run(torch, clusterer, poses, w), R.cluster(poses, w))


def test_no_particles(torch, clusterer):
    header, records, labels = run(torch, clusterer, np.zeros((0, 3)), None)
    assert tuple(header) == (0, 0, 0, 0, 0, 0.0) and records == [] and len(labels) == 0


def two_blobs(rng, gap_bins):
    """Blobs of weights 0.6 and 0.4 in the bin columns kx <= -1 and kx >= gap_bins, every bin of the
    band 0 .. gap_bins - 1 between them empty (all in heading bins 11 .. 12)."""
    n = 2000
    left = np.stack([-0.02 - 0.9 * rng.random(n), rng.random(n) - 0.5, 0.2 * rng.random(n) - 0.1], axis=1)
    right = np.stack([0.5 * gap_bins + 0.02 + 0.9 * rng.random(n), rng.random(n) - 0.5, 0.2 * rng.random(n) - 0.1], axis=1)
    wl, wr = rng.random(n) + 0.1, rng.random(n) + 0.1
    order = rng.permutation(2 * n)
    return np.concatenate([left, right])[order], np.concatenate([0.6 * wl / wl.sum(), 0.4 * wr / wr.sum()])[order]


def test_two_blobs_and_the_band_between_them(torch, clusterer):
    rng = np.random.default_rng(1)
    poses, w = two_blobs(rng, 2)
    want = R.cluster(poses, w)
    assert want["header"]["n_clusters"] == 2 and abs(want["records"][0]["W"] - 0.6) < 1e-12
    got = run(torch, clusterer, poses, w)
    compare(got, want)
    assert got[1][0].mean_x < 0.0 < got[1][1].mean_x
    # A band one bin wide: the bins either side of it differ by 2 in kx, which the contract's
    # adjacency (keys at most 1 apart) and the restatement keep apart: still two clusters.
    poses, w = two_blobs(rng, 1)
    want = R.cluster(poses, w)
    assert want["header"]["n_clusters"] == 2
    compare(run(torch, clusterer, poses, w), want)
    # no empty bin between them: bins -1 and 0 touch, the blobs are bridged into one cluster
    poses, w = two_blobs(rng, 0)
    want = R.cluster(poses, w)
    assert want["header"]["n_clusters"] == 1
    compare(run(torch, clusterer, poses, w), want)


def test_a_blob_across_plus_minus_pi(torch, clusterer):
    rng = np.random.default_rng(2)
    n = 3000
    theta = np.pi + 0.15 * rng.normal(size=n)
    theta = np.where(rng.random(n) < 0.5, theta, theta - 2.0 * np.pi)          # either side of the cut, unnormalised too
    poses = np.stack([1.2 + 0.1 * rng.normal(size=n), -0.7 + 0.1 * rng.normal(size=n), theta], axis=1)
    w = rng.random(n) + 0.1
    w /= w.sum()
    for n_theta in (24, 1):
        want = R.cluster(poses, w, n_theta=n_theta)
        assert want["header"]["n_clusters"] == 1 and abs(abs(want["records"][0]["mt"]) - np.pi) < 0.02
        got = run(torch, clusterer, poses, w, n_theta=n_theta)
        compare(got, want)
        assert got[1][0].var_theta < 0.05            # the spread round the mean, not round 0


def test_a_snake_and_a_comb(torch, clusterer):
    """300 bins in a line, one particle each, the smallest index at the far end and the others
    scrambled; and a comb: two arms of 60 bins two bins apart that join only at the tip."""
    rng = np.random.default_rng(3)
    snake = [(k, 40, 5) for k in range(300)]
    comb = [(k, 0, 5) for k in range(60)] + [(k, 2, 5) for k in range(60)] + [(60, 1, 5)]
    for name, shape in (("snake", snake), ("comb", comb)):
        order = np.concatenate([[len(shape) - 1], rng.permutation(len(shape) - 1)]) if name == "snake" else rng.permutation(len(shape))
        poses = in_bins(rng, len(shape), [shape[i] for i in order])
        w = np.full(len(shape), 1.0 / len(shape))
        want = R.cluster(poses, w)
        assert want["header"]["n_clusters"] == 1 and want["header"]["n_bins"] == len(shape)
        got = run(torch, clusterer, poses, w)
        compare(got, want)
        print("%s: B = %d, rounds = %d" % (name, got[0].n_bins, got[0].rounds))
        assert got[0].rounds <= got[0].n_bins + 1
    # both at once, with a second snake that stays apart
    shape = snake + comb + [(k, 44, 5) for k in range(100)]
    poses = in_bins(rng, len(shape), [shape[i] for i in rng.permutation(len(shape))])
    want = R.cluster(poses, None)
    assert want["header"]["n_clusters"] == 3
    got = run(torch, clusterer, poses, None)
    compare(got, want)
    assert got[0].rounds <= got[0].n_bins + 1


@pytest.mark.parametrize("bin_keys", [[(3, -2, 7)], [(3, -2, 7), (4, -2, 7)]], ids=["one bin", "two adjacent bins"])
def test_every_particle_in_one_or_two_bins(torch, clusterer, bin_keys):
    """The contention case: 100,000 particles in one bin, and in two adjacent bins."""
    n = 100000
    rng = np.random.default_rng(4)
    poses = in_bins(rng, n, bin_keys)
    want = R.cluster(poses, None)
    assert want["header"]["n_bins"] == len(bin_keys) and want["header"]["n_clusters"] == 1
    uniform = run(torch, clusterer, poses, None)
    compare(uniform, want)
    explicit = run(torch, clusterer, poses, np.full(n, 1.0 / n))
    compare(explicit, want)
    assert np.array_equal(uniform[2], explicit[2]) and raw_bytes(*uniform)[1] == raw_bytes(*explicit)[1]
    assert int(uniform[1][0].mass * 2.0 ** 40) == n * R.mass_q(1.0 / n)


def test_keys_that_share_one_slot_chain(torch, clusterer):
    """Five distinct keys whose hash has the same low bits in the table of this call (128 slots for
    40 particles), two of them differing only in the heading bin."""
    n_theta, n, mask = 360, 40, 127
    assert 2 * n <= mask + 1 and 2 * n > (mask + 1) // 2
    first = (5, -3, 10)
    chain = [first, (5, -3, 10 + 128)]
    home = R.key_hash(*first) & mask
    assert R.key_hash(*chain[1]) & mask == home
    for kx in range(-40, 40, 3):
        for ky in range(-40, 40, 3):
            if len(chain) < 5 and (kx, ky) != (5, -3) and R.key_hash(kx, ky, 200) & mask == home:
                chain.append((kx, ky, 200))
    assert len(chain) == 5 and len(set(chain)) == 5
    rng = np.random.default_rng(5)
    poses = in_bins(rng, n, chain, n_theta=n_theta)
    w = rng.random(n) + 0.1
    w /= w.sum()
    kx, ky, kt, out = R.keys(poses, w, n_theta=n_theta)
    assert not out.any() and {(int(a), int(b), int(c)) for a, b, c in zip(kx, ky, kt)} == set(chain)
    want = R.cluster(poses, w, n_theta=n_theta)
    assert want["header"]["n_bins"] == 5 and want["header"]["n_clusters"] == 5
    compare(run(torch, clusterer, poses, w, n_theta=n_theta), want)


def test_left_out_particles_of_every_kind(torch, clusterer):
    rng = np.random.default_rng(6)
    poses, w, _ = blobs(rng, 500, [(1.0, 1.0, 0.5), (1.6, 1.2, 0.6)])
    bad = {0: ("pose", (np.nan, 1.0, 0.5)), 7: ("pose", (1.0, np.inf, 0.5)), 64: ("pose", (1.0, 1.0, -np.inf)),
           65: ("pose", (0.5 * 2.0 ** 30, 1.0, 0.5)), 130: ("pose", (1.0, -1e300, 0.5)), 131: ("w", np.nan),
           255: ("w", -1e-9), 256: ("w", 1.0000001), 499: ("w", np.inf)}
    for i, (kind, value) in bad.items():
        if kind == "pose":
            poses[i] = value
        else:
            w[i] = value
    want = R.cluster(poses, w)
    assert want["header"]["n_left_out"] == len(bad) and want["labels"][0] == R.LEFT_OUT
    assert 0 not in [r["label"] for r in want["records"]]        # no label is taken from the particle left out
    got = run(torch, clusterer, poses, w)
    compare(got, want)
    assert all(got[2][i] == R.LEFT_OUT for i in bad) and sum(r.count for r in got[1]) + len(bad) == 500


def test_more_clusters_than_records_and_fewer(torch, clusterer):
    rng = np.random.default_rng(7)
    poses = in_bins(rng, 20, [(3 * k, -3 * k, (5 * k) % 24) for k in range(20)])
    w = rng.random(20) + 0.1
    w /= w.sum()
    want = R.cluster(poses, w, max_clusters=4)
    got = run(torch, clusterer, poses, w, max_clusters=4)
    compare(got, want, max_clusters=4)
    assert got[0].n_clusters == 20 and len(got[1]) == 4
    poses, w, _ = blobs(rng, 300, [(-5.0, 0.0, 0.0), (0.0, 5.0, 1.0), (5.0, 0.0, 2.0)], sigma=(0.1, 0.1, 0.05))
    want = R.cluster(poses, w, max_clusters=16)
    got = run(torch, clusterer, poses, w, max_clusters=16)
    compare(got, want, max_clusters=16)
    assert got[0].n_clusters == 3 and len(got[1]) == 3


def test_equal_mass_goes_by_label(torch, clusterer):
    """Two clusters of equal Q from different particle counts: 4 particles of weight 1/8 and 2 of
    weight 1/4 (exact in binary), and a lighter third."""
    rng = np.random.default_rng(8)
    keys = [(10, 0, 3)] + [(0, 0, 3)] * 2 + [(10, 0, 3)] * 3 + [(20, 5, 9)] * 2
    poses = np.stack([in_bins(rng, 1, [k])[0] for k in keys])
    w = np.array([0.125, 0.25, 0.25, 0.125, 0.125, 0.125, 0.0625, 0.0625])
    want = R.cluster(poses, w)
    assert [r["label"] for r in want["records"]] == [0, 1, 6] and want["records"][0]["Q"] == want["records"][1]["Q"]
    assert [r["count"] for r in want["records"]] == [4, 2, 2]
    compare(run(torch, clusterer, poses, w), want)
    # the same with the first two clusters' particles swapped: the order follows the labels
    swap = np.array([1, 0, 3, 2, 4, 5, 6, 7])
    want = R.cluster(poses[swap], w[swap])
    assert [r["count"] for r in want["records"]] == [2, 4, 2]
    compare(run(torch, clusterer, poses[swap], w[swap]), want)


def test_refusals_leave_the_object_as_it_was(torch, device):
    rng = np.random.default_rng(9)
    poses, w, _ = blobs(rng, 700, [(1.0, 1.0, 0.5), (-2.0, 3.0, -1.0)])
    fresh = Clusterer(device, 1000)
    want = raw_bytes(*run(torch, fresh, poses, w, 0.4, 0.6, 12, 3))
    fresh.close()
    c = Clusterer(device, 1000)
    d_p = torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()
    c.set_bins(0.4, 0.6, 12)
    c.set_max_clusters(3)
    refusals = [lambda: c.set_bins(float("nan"), 0.6, 12), lambda: c.set_bins(0.4, float("inf"), 12),
                lambda: c.set_bins(0.0, 0.6, 12), lambda: c.set_bins(0.4, -0.6, 12), lambda: c.set_bins(0.4, 0.6, 0),
                lambda: c.set_max_clusters(0), lambda: c.set_max_clusters(17),
                lambda: c.launch(d_p.data_ptr(), None, 1001), lambda: c.launch(None, None, 5)]
    for refuse in refusals:
        with pytest.raises(Ndt2dError) as ei:
            refuse()
        assert ei.value.code == _capi.ERR_INVALID
        d_w = torch.from_numpy(w).cuda()
        torch.cuda.synchronize()
        c.launch(d_p.data_ptr(), d_w.data_ptr(), 700)
        header, records = c.fetch_raw()
        got = raw_bytes(header, records, c.labels())
        assert got[1:] == want[1:]
    # a refused launch leaves the fetched result where it was
    with pytest.raises(Ndt2dError):
        c.launch(None, None, 5)
    header, records = c.fetch_raw()
    assert raw_bytes(header, records, c.labels())[1:] == want[1:]
    c.close()


def test_the_filters_estimate_is_the_heaviest_blob(torch, device):
    rng = np.random.default_rng(10)
    poses, w = two_blobs(rng, 6)
    f = ParticleFilter(500, 5000, MotionModel(0.1, 0.1, 0.1, 0.1, 0.05), device, seed=3)
    with torch.cuda.stream(f._stream):
        f.particles = torch.from_numpy(poses).to(f.device)
        f.weights = torch.from_numpy(w).to(f.device)
    f._update_statistics(have_moments=False)
    want = R.cluster(poses, w)
    kx, ky, kt, _ = R.keys(poses, w)
    occupied = {(int(a), int(b)) for a, b in zip(kx, ky)}
    mean = f.getMean()
    mkx, mky, _, _ = R.keys(mean.reshape(1, 3), np.array([0.5]))
    assert (int(mkx[0]), int(mky[0])) not in occupied          # the mean of the whole set lies in neither blob
    found = f.clusters()
    assert [c.label for c in found] == [r["label"] for r in want["records"]] and len(found) == 2
    assert f.cluster_header.n_clusters == 2 and f.cluster_header.n == len(poses)
    best = want["records"][0]
    est_mean, est_cov, share = f.estimate()
    a = best["abs"]
    assert abs(est_mean[0] - best["mx"]) <= BOUND * a["x"] / best["W"] and abs(est_mean[1] - best["my"]) <= BOUND * a["y"] / best["W"]
    assert abs(float(R.normalise_angle(est_mean[2] - best["mt"]))) <= 1e-12
    assert abs(est_cov[0, 0] - best["cxx"]) <= BOUND * a["xx"] / best["W"] and abs(est_cov[1, 1] - best["cyy"]) <= BOUND * a["yy"] / best["W"]
    assert abs(est_cov[0, 1] - best["cxy"]) <= BOUND * a["xy"] / best["W"] and est_cov[1, 0] == est_cov[0, 1]
    assert abs(est_cov[2, 2] - best["vt"]) <= BOUND * a["tt"] / best["W"]
    assert est_cov[0, 2] == est_cov[2, 0] == est_cov[1, 2] == est_cov[2, 1] == 0.0
    assert abs(share - 0.6) < 1e-12 and est_mean[0] < 0.0
    assert np.array_equal(f.getMean(), mean)                   # getMean is untouched


def test_global_localisation_ends_in_the_heaviest_cluster(torch):
    """The case of tests/seed_convergence_case.py, run as test_global_localisation_converges_on_the_truth
    (tests/test_gpu_seed.py) runs it.  At the end estimate()'s pose error is within the limits that
    test applies to the mean.  The heaviest cluster's share straight after init_global and at the end
    are printed, not asserted: they are unmeasured."""
    import seed_convergence_case as K
    params = K.matcher_params()
    scans = K.map_scans()
    m = ScanMatcherNDT(0)
    m.initialize("converge", **params)
    m.addScans(scans)
    occ = OccupancyMap(K.MAP_RESOLUTION, K.OCC_THRESH, m)
    occ.getMsg(K.occupancy_scans(scans))
    f = ParticleFilter(K.MIN_PARTICLES, K.N_PARTICLES, MotionModel(*K.ALPHAS), m, seed=K.SEED, resample_on="device")
    f.init_global(occ)
    first = f.clusters()
    first_header = f.cluster_header
    assert first_header.n == K.N_PARTICLES and first_header.n_left_out == 0
    steps = K.trajectory()
    for t, (truth, points) in enumerate(steps):
        f.update(*K.MOTION)
        f.measure(m, points)
        if t + 1 < len(steps):
            f.resample(K.KLD_ERR, K.KLD_Z)
    mean, cov, share = f.estimate()
    header = f.cluster_header
    labels = f._clusterer.labels()
    counts = np.bincount(labels[labels != R.LEFT_OUT].astype(np.int64), minlength=1)
    assert int(counts.sum()) + header.n_left_out == header.n == len(f.particles)
    assert int((counts > 0).sum()) == header.n_clusters
    err_xy, err_th = K.errors(mean, steps[-1][0])
    print("heaviest cluster: share %.4f of %d clusters (%d bins) after init_global; share %.4f of %d clusters at the end; "
          "position error %.4f m, heading error %.4f rad" %
          (first[0].share, first_header.n_clusters, first_header.n_bins, share, header.n_clusters, err_xy, err_th))
    assert err_xy <= params["ndt_resolution"]
    assert err_th < params["search_angular_size"]
    m.close()
