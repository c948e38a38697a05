"""Seeding that keeps off walls (Seeder.set_map / set_occupancy_map and ParticleFilter.init_global with
min_clearance) against the yardsticks: the table is np.flatnonzero((map == 0) & (d2 >= min_d2)) of
tests/clearance_restatement.py, the poses are tests/seed_restatement.py applied to that table, bit
for bit.  Without the clearance map none of the filtered tables can come out."""
import numpy as np
import pytest

import clearance_restatement as R
import seed_restatement as S
from ndt_2d_amd import MotionModel, OccupancyMap, ParticleFilter, ScanMatcherNDT, Seeder, synth

pytestmark = pytest.mark.gpu

GEO = (-3.35, 1.7, 0.05)          # origin_x, origin_y, resolution


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def device():
    m = ScanMatcherNDT(0)
    m.initialize("seed-clearance", **synth.matcher_params(1))
    m.addScans(synth.map_scans(1))
    return m


@pytest.fixture(scope="module")
def seeder(device):
    s = Seeder(device)
    yield s
    s.close()


@pytest.fixture(scope="module")
def big():
    """(300 x 300 map, its exact d2 without and with unknown cells as obstacles)"""
    grid = R.SHAPES["300x300 dense"]()
    return grid, R.d2_separable(grid), R.d2_separable(grid, True)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def poses_of(torch, seeder, n, seed, step, first=0):
    out = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    seeder.launch(out.data_ptr(), n, seed, step, first)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_a_corridor_three_cells_wide_keeps_its_centre_line(seeder):
    """Walls at rows 2 and 6, free rows 3 to 5: at 0.1 m (min_d2 = 4) only row 4 is two cells from
    both walls."""
    grid = np.full((9, 40), 100, dtype=np.int8)
    grid[3:6, :] = 0
    assert R.min_d2(0.1, 0.05) == 4
    plain = seeder.set_map(grid, *GEO)
    assert plain == 120
    count = seeder.set_map(grid, *GEO, min_clearance=0.1)
    want = R.cleared_table(grid, R.d2_separable(grid), 4)
    assert want.tolist() == list(range(4 * 40, 5 * 40))
    got = seeder.read_table()
    assert count == 40 < plain and got.dtype == np.uint32 and np.array_equal(got, want)
    # one cell more and nothing is left: F == 0 is no error of set_map
    assert seeder.set_map(grid, *GEO, min_clearance=0.15) == 0


def test_the_table_is_the_yardsticks_filtered_table(torch, seeder, big):
    grid, d2, d2_unknown = big
    plain = S.free_table(grid)
    for clearance, unknown in ((0.05, False), (0.15, False), (0.25, False), (0.3, False), (0.15, True)):
        threshold = R.min_d2(clearance, GEO[2])
        want = R.cleared_table(grid, d2_unknown if unknown else d2, threshold)
        count = seeder.set_map(grid, *GEO, min_clearance=clearance, unknown_is_obstacle=unknown)
        assert count == len(want) and np.array_equal(seeder.read_table(), want), (clearance, unknown)
        assert np.isin(want, plain).all()
        if threshold <= 1:
            assert np.array_equal(want, plain)          # every free cell is at least one cell from an obstacle
        else:
            assert 0 < len(want) < len(plain)           # strictly smaller: the band along the walls is gone
        # a device map through the clearance object of its own gives the same table
        d = torch.from_numpy(grid.copy()).cuda()
        torch.cuda.synchronize()
        from ndt_2d_amd import ClearanceMap
        cm = ClearanceMap(seeder._device)
        cm.compute_device(d.data_ptr(), 300, 300, unknown_is_obstacle=unknown)
        assert seeder.set_map_device(cm.mask(min_d2=threshold), 300, 300, *GEO) == len(want)
        assert np.array_equal(seeder.read_table(), want)
        cm.close()


def test_a_region_whose_nearest_obstacle_lies_outside_it(seeder):
    """The transform covers the whole map: the wall at column 30 empties the columns next to it,
    although the region ends at column 29."""
    grid = np.zeros((20, 40), dtype=np.int8)
    grid[:, 30] = 100
    region = (20, 5, 10, 10)                                           # columns 20 .. 29
    d2 = R.d2_separable(grid)
    want = R.cleared_table(grid, d2, 9, region)
    assert R.min_d2(0.15, 0.05) == 9
    assert len(want) == 10 * 8 and (want % 40).max() == 27              # columns 28 and 29 are 2 and 1 cells from it
    count = seeder.set_map(grid, *GEO, region=region, min_clearance=0.15)
    assert count == len(want) and np.array_equal(seeder.read_table(), want)
    assert count < seeder.set_map(grid, *GEO, region=region) == 100


def test_no_clearance_is_todays_call(torch, device, big):
    """min_clearance = 0.0: the table and the poses of the call without the argument, and no
    clearance object is made."""
    grid, _, _ = big
    a, b = Seeder(device), Seeder(device)
    assert a.set_map(grid, *GEO, region=(3, 4, 200, 250)) == b.set_map(grid, *GEO, region=(3, 4, 200, 250), min_clearance=0.0)
    assert np.array_equal(a.read_table(), b.read_table()) and np.array_equal(a.read_table(), S.free_table(grid, (3, 4, 200, 250)))
    assert same_bits(poses_of(torch, a, 1025, 7, 3), poses_of(torch, b, 1025, 7, 3))
    assert a._clearance is None and b._clearance is None
    b.set_map(grid, *GEO, min_clearance=0.1)
    assert b._clearance is not None
    a.close()
    b.close()


def test_filter_init_global_with_a_clearance_and_inject(torch, device):
    occ = OccupancyMap(0.05, 0.25, device)
    msg = occ.getMsg(synth.map_scans(1))
    grid = msg["data"]
    geo = (msg["origin_x"], msg["origin_y"], msg["resolution"])
    width = msg["width"]
    clearance = 0.2
    threshold = R.min_d2(clearance, geo[2])
    assert threshold == 16
    plain = S.free_table(grid)

    def new_filter():
        f = ParticleFilter(200, 5000, MotionModel(0.2, 0.2, 0.2, 0.2, 0.2), device, seed=23, resample_on="device")
        torch.cuda.synchronize()
        device.set_stream(f._stream.cuda_stream)
        return f

    for unknown in (False, True):
        d2 = R.d2_separable(grid, unknown)
        table = R.cleared_table(grid, d2, threshold)
        assert 100 < len(table) < len(plain)
        f = new_filter()
        f.init_global(occ, min_clearance=clearance, unknown_is_obstacle=unknown)       # the resident map
        p = f.particles.cpu().numpy()
        assert len(p) == 5000 and f._step == 2
        assert same_bits(p, S.sample(23, 1, 0, 5000, table, width, *geo))
        assert np.array_equal(f._seeder.read_table(), table)
        # every particle's cell has the clearance
        cx, cy = S.cell_of(p[:, 0], geo[0], geo[2]), S.cell_of(p[:, 1], geo[1], geo[2])
        assert np.all(grid[cy, cx] == 0) and np.all(d2[cy, cx].astype(np.int64) >= threshold)
        assert np.all(f.weights.cpu().numpy() == np.float64(1.0 / 5000))
        # the same map as an array
        g = new_filter()
        g.init_global((grid, *geo), min_clearance=clearance, unknown_is_obstacle=unknown)
        assert same_bits(g.particles.cpu().numpy(), p)
        # inject draws from the same table: steps 3 and 4
        torch.cuda.synchronize()
        device.set_stream(f._stream.cuda_stream)
        replaced = f.inject(0.3)
        want, take = S.inject(p, 0.3, 23, 3, 0, table, width, *geo)
        after = f.particles.cpu().numpy()
        assert replaced == int(take.sum()) > 1000 and same_bits(after, want)
        cx, cy = S.cell_of(after[:, 0], geo[0], geo[2]), S.cell_of(after[:, 1], geo[1], geo[2])
        assert np.all(d2[cy, cx].astype(np.int64) >= threshold)
        # a region and n
        region = (width // 2, 0, width - width // 2, msg["height"])
        f.init_global(occ, n=777, region=region, min_clearance=clearance, unknown_is_obstacle=unknown)
        assert same_bits(f.particles.cpu().numpy(),
                         S.sample(23, 5, 0, 777, R.cleared_table(grid, d2, threshold, region), width, *geo))
    # without the clearance the filter's call is what it was
    f = new_filter()
    f.init_global(occ)
    assert same_bits(f.particles.cpu().numpy(), S.sample(23, 1, 0, 5000, plain, width, *geo))
    assert f._seeder._clearance is None
    occ.close()
