"""Global localisation on the device (csrc/seed/ndt2d_seed.hip; Seeder, ParticleFilter.init_global /
inject) against the numpy restatement (tests/seed_restatement.py, itself pinned by
tests/test_seed_restatement.py) -- never against the device code itself.  The table is compared with
np.flatnonzero(map == 0), poses with np.array_equal on the float64 bits: no tolerance.

A tile of the table build is 256 cells and the scan's workgroup has 256 threads, so a region of more
than 65,536 cells gives some thread of the scan more than one tile: 300 x 300 (352 tiles) crosses
that boundary.  The streaming kernels' grid is capped at 4,096 blocks of 256 threads: 1,048,577
particles is the first size at which a thread takes a second particle."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import seed_restatement as S
from ndt_2d_amd import MotionModel, OccupancyMap, ParticleFilter, ScanMatcherNDT, Seeder, _capi, synth

pytestmark = pytest.mark.gpu

GEO = (-3.35, 1.7, 0.05)          # origin_x, origin_y, resolution
BEYOND_CAP = 4096 * 256 + 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def device():
    m = ScanMatcherNDT(0)
    m.initialize("seed", **synth.matcher_params(1))
    m.addScans(synth.map_scans(1))
    return m


@pytest.fixture(scope="module")
def seeder(device):
    """One seeder for the whole module, so that every table is also built in buffers that other
    sizes have used before it."""
    s = Seeder(device)
    yield s
    s.close()


@pytest.fixture(scope="module")
def world_map(device):
    """(OccupancyMap after one update of cfg-1's scans, its message)."""
    occ = OccupancyMap(0.05, 0.25, device)
    msg = occ.getMsg(synth.map_scans(1))
    return occ, msg


def random_map(height, width, seed, p_free=0.4):
    rng = np.random.default_rng(seed)
    values = np.array([0, -1, 100, 1, -128, 127, 2, -2], dtype=np.int8)
    pick = rng.random((height, width))
    grid = values[rng.integers(1, len(values), size=(height, width))]
    grid[pick < p_free] = 0
    return grid


def poses_of(torch, seeder, n, seed, step, first=0):
    out = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                  # (the seeder launches on the context's stream, not torch's)
    seeder.launch(out.data_ptr(), n, seed, step, first)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. the table ----------------------------------------------------------------------------

TABLE_CASES = {
    "1x1 free": (np.zeros((1, 1), dtype=np.int8), None),
    "1x1 unknown": (np.full((1, 1), -1, dtype=np.int8), None),
    "one free cell, the last": (np.pad(np.zeros((1, 1), dtype=np.int8), ((6, 0), (70, 0)), constant_values=100), None),
    "width 63": (random_map(5, 63, 63), None),
    "width 64": (random_map(4, 64, 64), None),
    "width 65": (random_map(9, 65, 65), None),
    "width 255": (random_map(3, 255, 255), None),
    "width 257": (random_map(7, 257, 257), None),
    "free cells in the last tile only": (np.concatenate([np.full(256 * 5, 100, dtype=np.int8),
                                                         random_map(1, 131, 3)[0]]).reshape(1, -1), None),
    "300 x 300: more tiles than the scan has threads": (random_map(300, 300, 300), None),
    "all free": (np.zeros((37, 41), dtype=np.int8), None),
    "none free": (np.full((37, 41), 100, dtype=np.int8), None),
    "stray values are not free": (np.array([[-1, 0, 100, 1, -128, 127, 0, 2]], dtype=np.int8), None),
    "region, low corner": (random_map(40, 70, 1), (0, 0, 9, 7)),
    "region, high corner": (random_map(40, 70, 2), (61, 33, 9, 7)),
    "region, one cell, the last": (random_map(40, 70, 3, p_free=1.0), (69, 39, 1, 1)),
    "region, a column": (random_map(300, 300, 4), (299, 0, 1, 300)),
    "region, whole map": (random_map(40, 70, 5), (0, 0, 70, 40)),
    "region, empty": (random_map(40, 70, 6), (3, 3, 0, 5)),
}


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_table_is_flatnonzero(torch, seeder, name):
    grid, region = TABLE_CASES[name]
    want = S.free_table(grid, region)
    if region is None:
        assert np.array_equal(want, np.flatnonzero(grid.reshape(-1) == 0))
    # the host-pointer form
    count = seeder.set_map(grid, *GEO, region=region)
    got = seeder.read_table()
    assert count == len(want) and got.dtype == np.uint32 and np.array_equal(got, want)
    # the device-pointer form agrees
    d = torch.from_numpy(grid.copy()).cuda()
    torch.cuda.synchronize()
    count = seeder.set_map_device(d.data_ptr(), grid.shape[1], grid.shape[0], *GEO, region=region)
    assert count == len(want) and np.array_equal(seeder.read_table(), want)
    if len(want) == 0:
        # F == 0 is no error of set_map; a sample call has no free cell
        out = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for call in (lambda: seeder.launch(out.data_ptr(), 4, 1, 1),
                     lambda: seeder.inject_launch(out.data_ptr(), 4, 0.5, 1, 1)):
            with pytest.raises(_capi.Ndt2dError) as ei:
                call()
            assert ei.value.code == _capi.ERR_STATE and "no free cell" in str(ei.value)
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()


def test_resident_map_against_its_own_read(torch, device, seeder, world_map):
    """An OccupancyMap after an update: the table of its resident map (nothing uploaded) is the
    table of the array its read gives."""
    occ, msg = world_map
    grid = msg["data"]
    assert set(np.unique(grid).tolist()) == {-1, 0, 100}
    ptr, info = occ.device_map()
    assert ptr and (info.width, info.height) == (msg["width"], msg["height"])
    assert (info.origin_x, info.origin_y, info.resolution) == (msg["origin_x"], msg["origin_y"], msg["resolution"])
    count = seeder.set_occupancy_map(occ)
    want = np.flatnonzero(grid.reshape(-1) == 0)
    assert count == len(want) > 1000 and np.array_equal(seeder.read_table(), want)
    resident = poses_of(torch, seeder, 1025, 3, 4)
    seeder.set_map(grid, msg["origin_x"], msg["origin_y"], msg["resolution"])
    assert np.array_equal(seeder.read_table(), want)
    assert same_bits(poses_of(torch, seeder, 1025, 3, 4), resident)
    region = (msg["width"] // 2, msg["height"] // 2, msg["width"] - msg["width"] // 2, msg["height"] - msg["height"] // 2)
    assert seeder.set_occupancy_map(occ, region) == len(S.free_table(grid, region))
    assert np.array_equal(seeder.read_table(), S.free_table(grid, region))
    # before the first update there is no resident map
    fresh = OccupancyMap(0.05, 0.25, device)
    with pytest.raises(_capi.Ndt2dError) as ei:
        fresh.device_map()
    assert ei.value.code == _capi.ERR_STATE
    fresh.close()


# ---- 2. samples --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample_map():
    grid = random_map(300, 257, 11)
    region = (5, 9, 250, 280)
    return grid, region, S.free_table(grid, region)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, BEYOND_CAP])
def test_samples_are_the_restatements_bits(torch, seeder, sample_map, n):
    grid, region, table = sample_map
    assert seeder.set_map(grid, *GEO, region=region) == len(table)
    seed, step, first = 0x1234567890abcdef, 41, (1 << 32) - 7        # the index crosses 2^32
    got = poses_of(torch, seeder, n, seed, step, first)
    want = S.sample(seed, step, first, n, table, grid.shape[1], *GEO)
    assert same_bits(got, want)
    # the same call twice
    assert same_bits(poses_of(torch, seeder, n, seed, step, first), got)
    # shards draw what the whole set would
    if n > 1:
        half = n // 2
        lo = poses_of(torch, seeder, half, seed, step, first)
        hi = poses_of(torch, seeder, n - half, seed, step, first + half)
        assert same_bits(np.concatenate([lo, hi]), got)
    # every pose lies in a free cell, in the region, with theta in [-pi, pi)
    cx, cy = S.cell_of(got[:, 0], GEO[0], GEO[2]), S.cell_of(got[:, 1], GEO[1], GEO[2])
    assert np.all(grid[cy, cx] == 0)
    x0, y0, w, h = region
    assert np.all((cx >= x0) & (cx < x0 + w) & (cy >= y0) & (cy < y0 + h))
    assert np.all((got[:, 2] >= -np.pi) & (got[:, 2] < np.pi))


def test_samples_at_the_ends_of_the_counters(torch, seeder, sample_map):
    """The known-answer counters: seed, step and index all-ones (step + 1 and the index wrap)."""
    grid, region, table = sample_map
    seeder.set_map(grid, *GEO, region=region)
    top = (1 << 64) - 1
    for seed, step, first in ((0, 0, 0), (top, top, top), (top, top - 1, top - 2)):
        got = poses_of(torch, seeder, 5, seed, step, first)
        assert same_bits(got, S.sample(seed, step, first, 5, table, grid.shape[1], *GEO))


# ---- 3. inject ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 65, 1025, BEYOND_CAP])
@pytest.mark.parametrize("probability", [0.0, 0.3, 1.0])
def test_inject_replaces_exactly_the_restatements_set(torch, seeder, sample_map, n, probability):
    grid, region, table = sample_map
    seeder.set_map(grid, *GEO, region=region)
    seed, step, first = 99, 7, 12345
    rng = np.random.default_rng(n)
    before = rng.normal(size=(n, 3))
    before[::3] = -0.0                                              # the sign of a zero is kept
    weights = rng.random(n)
    d_p = torch.from_numpy(before.copy()).cuda()
    d_w = torch.from_numpy(weights.copy()).cuda()
    d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    seeder.inject_launch(d_p.data_ptr(), n, probability, seed, step, first, d_count.data_ptr())
    torch.cuda.synchronize()
    want, take = S.inject(before, probability, seed, step, first, table, grid.shape[1], *GEO)
    got = d_p.cpu().numpy()
    assert same_bits(got, want)                                     # untouched particles keep their bits
    assert int(d_count.item()) == int(take.sum())                   # the count is exact
    assert np.array_equal(d_w.cpu().numpy(), weights)               # weights are not touched
    if probability == 0.0:
        assert not take.any() and same_bits(got, before)
    if probability == 1.0:
        assert take.all() and same_bits(got, poses_of(torch, seeder, n, seed, step, first))
    # without a count the poses are the same
    d_q = torch.from_numpy(before.copy()).cuda()
    torch.cuda.synchronize()
    seeder.inject_launch(d_q.data_ptr(), n, probability, seed, step, first, None)
    torch.cuda.synchronize()
    assert same_bits(d_q.cpu().numpy(), want)


# ---- 4. refusals -------------------------------------------------------------------------------

def test_refusals_leave_the_object_as_it_was(torch, device):
    L = _capi.lib()
    h = device.device_handle
    s = C.c_void_p()
    assert L.ndt2d_seed_create(h, None) == _capi.ERR_INVALID
    assert L.ndt2d_seed_create(None, C.byref(s)) == _capi.ERR_INVALID and not s.value
    n_out = C.c_size_t(0)
    ms = C.c_float(0.0)
    grid = np.zeros((4, 6), dtype=np.int8)
    p = grid.ctypes.data_as(C.c_void_p)
    for rc in (L.ndt2d_seed_destroy(None), L.ndt2d_seed_set_map(None, p, 6, 4, 0.0, 0.0, 0.1, None),
               L.ndt2d_seed_set_map_device(None, p, 6, 4, 0.0, 0.0, 0.1, None), L.ndt2d_seed_free_count(None, C.byref(n_out)),
               L.ndt2d_seed_read_table(None, None, 0, C.byref(n_out)), L.ndt2d_seed_launch(None, None, 0, 0, 0, 0),
               L.ndt2d_seed_inject_launch(None, None, 0, 0.5, 0, 0, 0, None), L.ndt2d_seed_set_timing(None, 1),
               L.ndt2d_seed_last_ms(None, C.byref(ms), C.byref(ms))):
        assert rc == _capi.ERR_INVALID
    assert L.ndt2d_seed_last_error(None) == b""

    seeder = Seeder(device)
    out = torch.zeros((8, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def refused(call, code, text):
        with pytest.raises(_capi.Ndt2dError) as ei:
            call()
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    # no map yet
    refused(lambda: seeder.free_count(), _capi.ERR_STATE, "no map")
    refused(lambda: seeder.read_table(), _capi.ERR_STATE, "no map")
    refused(lambda: seeder.launch(out.data_ptr(), 8, 1, 1), _capi.ERR_STATE, "no map")
    refused(lambda: seeder.inject_launch(out.data_ptr(), 8, 0.5, 1, 1), _capi.ERR_STATE, "no map")
    refused(lambda: seeder.last_ms(), _capi.ERR_STATE, "no timed launch")

    grid = random_map(20, 30, 8)
    table = S.free_table(grid)
    assert seeder.set_map(grid, *GEO) == len(table)
    before = poses_of(torch, seeder, 100, 5, 6)
    d = torch.from_numpy(grid.copy()).cuda()
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    for form in ("host", "device"):
        def set_map(width, height, ox, oy, res, region=None, null=False):
            ptr = None if null else (grid.ctypes.data_as(C.c_void_p) if form == "host" else d.data_ptr())
            fn = L.ndt2d_seed_set_map if form == "host" else L.ndt2d_seed_set_map_device
            reg = (C.c_uint32 * 4)(*region) if region is not None else None
            rc = fn(seeder._s, ptr, width, height, ox, oy, res, reg)
            return rc, L.ndt2d_seed_last_error(seeder._s).decode()

        for args, word in (((30, 20, 0.0, 0.0, 0.1, None, True), "null map"),
                           ((0, 20, 0.0, 0.0, 0.1), "width * height"), ((30, 0, 0.0, 0.0, 0.1), "width * height"),
                           ((1 << 16, 1 << 15, 0.0, 0.0, 0.1), "width * height"),
                           ((0xffffffff, 0xffffffff, 0.0, 0.0, 0.1), "width * height"),
                           ((30, 20, 0.0, 0.0, 0.0), "resolution"), ((30, 20, 0.0, 0.0, -0.1), "resolution"),
                           ((30, 20, 0.0, 0.0, nan), "resolution"), ((30, 20, 0.0, 0.0, inf), "resolution"),
                           ((30, 20, nan, 0.0, 0.1), "origin"), ((30, 20, 0.0, -inf, 0.1), "origin"),
                           ((30, 20, 0.0, 0.0, 0.1, (25, 0, 6, 1)), "region"), ((30, 20, 0.0, 0.0, 0.1, (0, 19, 1, 2)), "region"),
                           ((30, 20, 0.0, 0.0, 0.1, (0xffffffff, 0, 2, 1)), "region"),
                           ((30, 20, 0.0, 0.0, 0.1, (31, 0, 0, 0)), "region")):
            rc, msg = set_map(*args)
            assert rc == _capi.ERR_INVALID and word in msg, (form, args, rc, msg)
            # the table, the geometry and the samples are those of the accepted map
            assert seeder.free_count() == len(table) and np.array_equal(seeder.read_table(), table)
            assert same_bits(poses_of(torch, seeder, 100, 5, 6), before)
    # the sample calls
    refused(lambda: seeder.launch(None, 8, 1, 1), _capi.ERR_INVALID, "null poses")
    refused(lambda: seeder.inject_launch(None, 8, 0.5, 1, 1), _capi.ERR_INVALID, "null poses")
    for bad in (-0.001, 1.0000001, nan, inf, -inf):
        refused(lambda: seeder.inject_launch(out.data_ptr(), 8, bad, 1, 1), _capi.ERR_INVALID, "probability")
    small = np.empty(3, dtype=np.uint32)
    rc = L.ndt2d_seed_read_table(seeder._s, small.ctypes.data_as(C.POINTER(C.c_uint32)), 3, C.byref(n_out))
    assert rc == _capi.ERR_INVALID and n_out.value == len(table)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                               # no refused call wrote a pose
    # n == 0 is accepted and writes nothing
    seeder.launch(None, 0, 1, 1)
    seeder.inject_launch(None, 0, 0.5, 1, 1)
    assert same_bits(poses_of(torch, seeder, 100, 5, 6), before)
    # the timer
    seeder.set_timing(True)
    seeder.set_map(grid, *GEO)
    poses_of(torch, seeder, 100, 5, 6)
    table_ms, sample_ms = seeder.last_ms()
    assert table_ms > 0.0 and sample_ms > 0.0
    seeder.set_timing(False)
    seeder.close()


# ---- 5. the filter -----------------------------------------------------------------------------

def test_filter_init_global_inject_and_a_round(torch, device, world_map):
    occ, msg = world_map
    grid = msg["data"]
    table = np.flatnonzero(grid.reshape(-1) == 0)
    geo = (msg["origin_x"], msg["origin_y"], msg["resolution"])
    _, pts, _ = synth.query_scan(1)

    def new_filter():
        return ParticleFilter(200, 6000, MotionModel(0.2, 0.2, 0.2, 0.2, 0.2), device, seed=17, resample_on="device")

    def use(f):
        """A filter's kernels run on the stream the context is bound to: one filter at a time."""
        torch.cuda.synchronize()
        device.set_stream(f._stream.cuda_stream)
        return f

    a, b = new_filter(), new_filter()
    use(a).init_global(occ)                                          # the resident map
    use(b).init_global((grid, *geo))                                 # the same map as an array
    pa, pb = a.particles.cpu().numpy(), b.particles.cpu().numpy()
    assert len(a.particles) == len(b.particles) == 6000 and same_bits(pa, pb)
    # the first call of a new filter: steps 1 and 2 of its counter
    assert same_bits(pa, S.sample(17, 1, 0, 6000, table, msg["width"], *geo)) and a._step == 2
    wa = a.weights.cpu().numpy()
    assert wa.shape == (6000,) and np.all(wa == np.float64(1.0 / 6000))
    # the statistics are updateStatistics' of that set with those weights (the oracle's; smoke()'s bounds)
    _, mean, cov = O.pf_update_statistics(pa, wa)
    assert np.allclose(a.getMean(), mean, rtol=1e-9, atol=1e-12)
    assert np.allclose(a.getCovariance()[:2, :2], cov[:2, :2], rtol=1e-8, atol=1e-12)
    assert np.array_equal(a.getMean(), b.getMean())
    # n and a region
    region = (msg["width"] // 2, 0, msg["width"] - msg["width"] // 2, msg["height"])
    b.init_global(occ, n=777, region=region)
    assert len(b.particles) == 777 and b._step == 4
    assert same_bits(b.particles.cpu().numpy(), S.sample(17, 3, 0, 777, S.free_table(grid, region), msg["width"], *geo))
    assert np.all(b.weights.cpu().numpy() == np.float64(1.0 / 777))
    assert np.all(S.cell_of(b.particles.cpu().numpy()[:, 0], geo[0], geo[2]) >= region[0])

    # inject: steps 3 and 4, the restatement's set and count, weights untouched
    assert use(a).mean_measure_weight() is None
    a.measure(device, pts)
    # the mean unnormalised weight: the oracle's scores of the same set (each within the project's
    # score bound of 1e-12, so their mean is too); negative, as the reference's scores are
    ref = O.ScanMatcherNDT()
    ref.initialize(**synth.matcher_params(1))
    ref.addScans(synth.map_scans(1))
    w_avg = float(O.pf_measure(ref, pa, pts).sum()) / 6000
    assert w_avg < 0.0 and abs(a.mean_measure_weight() - w_avg) <= 1e-12
    w_before = a.weights.cpu().numpy()
    replaced = a.inject(0.25)
    want, take = S.inject(pa, 0.25, 17, 3, 0, table, msg["width"], *geo)
    assert replaced == int(take.sum()) and 0.2 * 6000 < replaced < 0.3 * 6000 and a._step == 4
    assert same_bits(a.particles.cpu().numpy(), want)
    assert np.array_equal(a.weights.cpu().numpy(), w_before)
    assert a.inject(0.0) == 0 and a._step == 6 and same_bits(a.particles.cpu().numpy(), want)
    # a filter that was never seeded has no table
    with pytest.raises(_capi.Ndt2dError) as ei:
        use(new_filter()).inject(0.1)
    assert ei.value.code == _capi.ERR_STATE

    # a round after init_global: measure, resample on the device, measure
    c = use(new_filter())
    c.init_global(occ)
    c.measure(device, pts)
    c.resample(0.01, 2.3)
    assert c.min_particles <= len(c.particles) <= c.max_particles
    c.measure(device, pts)
    assert np.all(np.isfinite(c.getMean())) and abs(c.weights.sum().item() - 1.0) < 1e-9
    assert c.min_particles <= len(c.particles) <= c.max_particles


# ---- 6. convergence: a condition, not a timing ---------------------------------------------------

def test_global_localisation_converges_on_the_truth(torch):
    """The case of tests/seed_convergence_case.py: the generator's smallest world with a map of one
    corner only (three scans on an L, range_max 2.5 m), 20,000 particles seeded over its free
    space, ten steps of update / measure / resample on the device.  The filter's mean ends within
    one ndt_resolution of the true position and its heading within search_angular_size.

    The CPU restatement of the same loop (tests/test_seed_convergence_host.py) ends 0.0264 m and
    0.0076 rad from the truth.  The device's scores differ from the oracle's by up to 1e-12, so the
    two runs need not draw the same particles: each is held to the truth, not to the other."""
    import seed_convergence_case as K
    params = K.matcher_params()
    scans = K.map_scans()
    m = ScanMatcherNDT(0)
    m.initialize("converge", **params)
    m.addScans(scans)
    occ = OccupancyMap(K.MAP_RESOLUTION, K.OCC_THRESH, m)
    msg = occ.getMsg(K.occupancy_scans(scans))
    f = ParticleFilter(K.MIN_PARTICLES, K.N_PARTICLES, MotionModel(*K.ALPHAS), m, seed=K.SEED, resample_on="device")
    f.init_global(occ)
    assert len(f.particles) == K.N_PARTICLES
    # (the seeded set is the restatement's: the loop starts from the same particles as the CPU's)
    assert same_bits(f.particles.cpu().numpy(),
                     S.sample(K.SEED, 1, 0, K.N_PARTICLES, np.flatnonzero(msg["data"].reshape(-1) == 0), msg["width"],
                              msg["origin_x"], msg["origin_y"], msg["resolution"]))
    steps = K.trajectory()
    sizes = []
    for t, (truth, points) in enumerate(steps):
        f.update(*K.MOTION)
        f.measure(m, points)
        if t + 1 < len(steps):
            f.resample(K.KLD_ERR, K.KLD_Z)
            sizes.append(len(f.particles))
    err_xy, err_th = K.errors(f.getMean(), steps[-1][0])
    print("device filter: position error %.4f m, heading error %.4f rad, sizes %s" % (err_xy, err_th, sizes))
    assert err_xy <= params["ndt_resolution"]
    assert err_th < params["search_angular_size"]
    assert all(K.MIN_PARTICLES <= n <= K.N_PARTICLES for n in sizes) and sizes[-1] < K.N_PARTICLES
    m.close()
