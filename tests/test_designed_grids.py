"""The designed grids (tests/designed_grids.py) on the CPU: the vectors, the constructions and the
test's own reference are validated here, before any GPU sees them.

  * the oracle's likelihood on the rank-one grid is math.exp(e) bit for bit: the construction
    delivers exactly the intended exponent;
  * glibc's exp against `decimal` over the whole vector set: at most 1 ulp / 1 subnormal unit
    (so the caps the GPU tests hold the kernels to, 2 and 2, are ones the reference itself meets
    with room to spare);
  * `decimal` against mpmath on a sample (the reference of the reference);
  * the cells6 import of the oracle is the inverse of its export;
  * the numpy restatements of record_exponent and getIndex agree with the oracle on the
    part-B and part-C grids, bit for bit and index for index.
"""
import math

import numpy as np
import pytest

import designed_grids as D
import oracle_lib as O
from ndt_2d_amd import synth


@pytest.fixture(scope="module")
def vectors():
    return D.exponent_vectors()


@pytest.fixture(scope="module")
def reference(vectors):
    ok = D.classify(vectors)[0]
    return ok, D.exp_reference(vectors[ok])


def _same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def test_vector_set_has_its_classes(vectors):
    ok, zero, inf, nan = D.classify(vectors)
    assert 60000 <= len(vectors) <= 62000
    assert nan.sum() == 1 and zero.sum() > 30 and inf.sum() > 5
    v = vectors[ok]
    assert ((v > -745.14) & (v < -708.4)).sum() > 6000            # subnormal results
    assert (v > 0).sum() > 6000 and D.EXP_OVERFLOW_ABOVE in v
    assert np.nextafter(D.EXP_OVERFLOW_ABOVE, np.inf) in vectors[inf]
    for special in (0.0, -1000.0, -1e300, -np.inf, np.inf, 1e300, 1e15, 5e-324, -5e-324, 2.0 ** -53):
        assert special in vectors
    assert np.signbit(vectors[vectors == 0.0]).any() and not np.signbit(vectors[vectors == 0.0]).all()
    # a rint tie of the range reduction: x log2(e) within 2^-40 of k + 1/2, for many k
    t = vectors[ok] * 1.4426950408889634
    assert (np.abs(t - np.floor(t) - 0.5) < 2.0 ** -40).sum() > 1500


@pytest.mark.parametrize("cell_size", [4.0, 3.0])
def test_rank_one_grid_delivers_the_exponent_exactly(vectors, cell_size):
    """Oracle likelihood at the probe point of every cell == math.exp(e), bit for bit: -0.0, +-inf,
    NaN, 5e-324 and 1e300 included; and the numpy record_exponent gives e itself."""
    n = 0
    for lat, which in D.vector_chunks(vectors, 128, cell_size):
        ndt = O.NDT.from_cells6(*lat.grid)
        pts = lat.points(1)[:, 0, :]
        use = np.flatnonzero(which >= 0)
        e = vectors[which[use]]
        idx = D.get_index(pts[use, 0], pts[use, 1], lat.size_x, lat.size_y, lat.cell_size, lat.origin)
        got_e = D.record_exponent(lat.cells6[idx], pts[use, 0], pts[use, 1])
        same_e = _same_bits(got_e, e) | ((e == 0.0) & (got_e == 0.0))     # (-0.0 * 1 + 0 = +0.0)
        assert same_e.all(), e[~same_e][:5]
        got = np.array([ndt.likelihood_point(x, y) for x, y in pts[use]])
        with np.errstate(over="ignore"):
            want = np.array([math.exp(v) if v <= D.EXP_OVERFLOW_ABOVE else (v if v != v else np.inf)
                             for v in e])
        assert _same_bits(got, want).all(), e[~_same_bits(got, want)][:5]
        assert np.array_equal(lat.candidate_exponents(1)[use, 0], e, equal_nan=True)
        n += len(use)
    assert n == len(vectors)


def test_isotropic_grid_delivers_the_exponent_exactly(vectors):
    v = vectors[np.isfinite(vectors) & (vectors < 0.0)][::7]
    for cell_size in (4.0, 3.0):
        for lat, which in D.vector_chunks(v, 32, cell_size, "iso"):
            ndt = O.NDT.from_cells6(*lat.grid)
            pts = lat.points(1)[:, 0, :]
            use = np.flatnonzero(which >= 0)
            got = np.array([ndt.likelihood_point(x, y) for x, y in pts[use]])
            want = np.array([math.exp(e) for e in v[which[use]]])
            assert _same_bits(got, want).all()


def test_glibc_exp_against_decimal(vectors, reference):
    """The reference's own error on the vector set: at most 1 ulp for normal results, at most 1
    unit of 2^-1074 for subnormal ones (measured: 0.505 and 0.500)."""
    ok, ref = reference
    got = np.array([math.exp(x) for x in vectors[ok]])
    err = ref.error(got)
    worst_normal = float(err[ref.normal].max())
    worst_sub = float(err[~ref.normal].max())
    print("glibc exp against decimal: %.4f ulp (normal, %d values), %.4f units (subnormal, %d values)"
          % (worst_normal, ref.normal.sum(), worst_sub, (~ref.normal).sum()))
    assert worst_normal <= 1.0 and worst_sub <= 1.0
    assert (~ref.normal).sum() > 6000
    # RN(exp) itself is monotone and is what float(Decimal) gives
    order = np.argsort(vectors[ok], kind="stable")
    assert np.all(np.diff(ref.y[order]) >= 0.0)
    # the two scalar helpers say the same
    assert D.ulp_error(math.exp(-3.25), -3.25) <= 0.51 and D.ulp_error(np.nextafter(math.exp(-3.25), 1.0), -3.25) > 0.49
    assert D.subnormal_units(math.exp(-720.5), -720.5) <= 0.5
    # special values of the reference's exp, as the GPU tests expect them of the kernels
    _, zero, inf, _ = D.classify(vectors)
    assert all(math.exp(x) == 0.0 for x in vectors[zero])
    assert math.exp(D.EXP_OVERFLOW_ABOVE) < np.inf
    with pytest.raises(OverflowError):
        math.exp(float(np.nextafter(D.EXP_OVERFLOW_ABOVE, np.inf)))


def test_decimal_against_mpmath(vectors, reference):
    """The test's own reference: decimal at 50 digits against mpmath at 200 bits, on a sample."""
    mpmath = pytest.importorskip("mpmath")
    from decimal import Decimal, localcontext
    ok, ref = reference
    v = vectors[ok]
    pick = np.random.default_rng(2).choice(len(v), 3000, replace=False)
    pick = np.concatenate([pick, np.flatnonzero(v == D.EXP_OVERFLOW_ABOVE), np.flatnonzero(v == -745.1332191019411)])
    with mpmath.workprec(200), localcontext() as ctx:
        ctx.prec = D.PREC
        for i in pick:
            m = mpmath.exp(mpmath.mpf(float(v[i])))
            d = ref.values[i]
            rel = abs(Decimal(mpmath.nstr(m, 60, strip_zeros=False, min_fixed=0, max_fixed=0)) - d) / d
            assert rel < Decimal("1e-45"), (v[i], rel)


def test_cells6_round_trip():
    """export -> import -> export of a built cfg-1 grid, bit for bit, NaN cells included; and the
    imported grid scores as the built one."""
    scans = synth.map_scans(1)
    ref = O.ScanMatcherNDT()
    ref.initialize(**synth.matcher_params(1))
    ref.addScans(scans)
    ndt = ref.ndt
    a = ndt.cells6()
    a[7] = [np.nan, 0.5, np.nan, 1.0, np.inf, 9.0]            # (a NaN cell of our own as well)
    back = O.NDT.from_cells6(a, ndt.size_x, ndt.size_y, ndt.cell_size, ndt.origin)
    b = back.cells6()
    assert _same_bits(a, b).all()
    assert (back.size_x, back.size_y, back.cell_size, back.origin) == (ndt.size_x, ndt.size_y, ndt.cell_size, ndt.origin)
    a = ndt.cells6()
    twin = O.ScanMatcherNDT()
    twin.initialize(**synth.matcher_params(1))
    twin.setCells6(a, ndt.size_x, ndt.size_y, ndt.cell_size, ndt.origin)
    assert _same_bits(twin.ndt.cells6(), a).all()
    guess, pts, _ = synth.query_scan(1)
    for pose in (guess, (0.3, -0.2, 1.0)):
        assert twin.scorePoints(pts, pose) == ref.scorePoints(pts, pose)


@pytest.mark.parametrize("shape", ["rank1", "iso"])
def test_numpy_record_exponent_agrees_with_the_oracle_on_the_skip_rows(shape):
    """Part B's grids: exp(numpy record_exponent) == the oracle's likelihood bit for bit at every
    beam end point, and the exponent is the row's (the construction is exact there too)."""
    rows = D.skip_rows(shape) + (D.level_rows() if shape == "iso" else [])
    assert len(rows) > 1000
    n = 0
    for cell_size in (4.0, 3.0):
        for lat, part, n_beams in list(D.rows_lattices(rows, cell_size, shape))[::5]:
            ndt = O.NDT.from_cells6(*lat.grid)
            pts = lat.points(n_beams).reshape(-1, 2)
            want_e = lat.candidate_exponents(n_beams).ravel()
            idx = D.get_index(pts[:, 0], pts[:, 1], lat.size_x, lat.size_y, lat.cell_size, lat.origin)
            oracle_idx = np.array([ndt.getIndex(x, y) for x, y in pts])
            assert np.array_equal(idx, oracle_idx)
            hit = (idx >= 0) & (lat.cells6[np.maximum(idx, 0), 5] >= 5.0)
            assert np.array_equal(hit, np.isfinite(want_e) | (want_e > 0))
            e = D.record_exponent(lat.cells6[idx[hit]], pts[hit, 0], pts[hit, 1])
            assert _same_bits(e, want_e[hit]).all()
            like = np.array([ndt.likelihood_point(x, y) for x, y in pts[hit]])
            assert _same_bits(like, np.array([math.exp(v) for v in e])).all()
            assert all(ndt.likelihood_point(x, y) == 0.0 for x, y in pts[~hit][:200])
            n += int(hit.sum())
    assert n > 2000


def test_skip_probes_straddle_the_thresholds():
    """The probes of part B lie either side of the kernel's bound and of the true half-ulp
    threshold of every carrier sum -- and the kernel's bound is the conservative one."""
    for name, carriers in D.skip_carriers().items():
        s = D.carrier_sum(carriers)
        bound = D.kernel_negligible_below(s)
        probes = D.skip_probes(s)
        half_ulp = 0.5 * (np.nextafter(s, np.inf) - s)
        t = np.array([float(D.decimal_exp(p)) for p in probes])
        assert (probes < bound).any() and (probes > bound).any(), name
        if s > 1e-300:
            assert (t < half_ulp).any() and (t > half_ulp).any(), name
            # what the kernel may skip changes nothing: RN(s + t) == s
            assert all(s + ti == s for ti, p in zip(t, probes) if p < bound), name
        assert bound == -746.0 or bound <= math.log(s) - 37.43 + 1e-9 or s < 1e-300, name
    assert D.kernel_negligible_below(1.0) == -38.0 and D.kernel_negligible_below(0.0) == -746.0


@pytest.mark.parametrize("cell_size,origin", [(4.0, (0.0, 0.0)), (4.0, (-9.0, 6.5)), (3.0, (-4.5, 1.5)),
                                              (0.3, (-0.7, 0.45)), (0.1, (-0.7, 0.45)), (0.1, (0.0, 0.0))])
def test_checkerboard_indices_agree_with_the_oracle(cell_size, origin):
    """Part C's grids: numpy getIndex == the oracle's, index for index, at every probe coordinate
    of either axis; a wrong cell is worth at least 0.5; the probes hold points inside the lane
    kernels' guard band and points just outside it; for cell sizes that are not powers of two
    they hold quotients that round across an integer."""
    board = D.Checkerboard(cell_size, origin)
    ndt = O.NDT.from_cells6(*board.grid)
    xs, ys = board.coordinates(0), board.coordinates(1)
    mid_x, mid_y = origin[0] + 2.5 * cell_size, origin[1] + 3.5 * cell_size
    got_x = D.get_index(xs, np.full(len(xs), mid_y), board.size_x, board.size_y, cell_size, origin)
    got_y = D.get_index(np.full(len(ys), mid_x), ys, board.size_x, board.size_y, cell_size, origin)
    assert np.array_equal(got_x, [ndt.getIndex(x, mid_y) for x in xs])
    assert np.array_equal(got_y, [ndt.getIndex(mid_x, y) for y in ys])
    assert (got_x < 0).sum() >= 20 and (got_x >= 0).sum() > 200
    # the origin itself is inside, the double below it is not; the far edge is outside, the double below it inside
    o, far = origin[0], board.boundaries(0)[-1]
    assert ndt.getIndex(o, mid_y) >= 0 and ndt.getIndex(np.nextafter(o, -np.inf), mid_y) < 0
    if (far - o) / cell_size >= board.size_x:
        assert ndt.getIndex(far, mid_y) < 0
    # terms: the numpy expectation against the oracle's likelihood on a sample of points
    rng = np.random.default_rng(4)
    px, py = rng.choice(xs, 1500), rng.choice(ys, 1500)
    want = board.expected_terms(px, py)
    got = np.array([ndt.likelihood_point(x, y) for x, y in zip(px, py)])
    assert np.max(np.abs(got - want)) < 1e-25
    # neighbours along either axis differ by more than 0.5 (checked on the cells' kinds)
    k = board.kind.reshape(board.size_y, board.size_x)
    one = k == 1
    diff_x = (one[:, :-2] != one[:, 1:-1])
    diff_y = (one[:-2, :] != one[1:-1, :])
    assert diff_x.mean() > 0.7 and diff_y.mean() > 0.7
    for axis, coords in ((0, xs), (1, ys)):
        for sub_log2 in (0, 1, 2):
            inside, outside = D.band_counts(board, coords, axis, sub_log2)
            assert inside > 0 and outside > 0, (axis, sub_log2, inside, outside)
        # 2, 3 and 4 units of 2^-16 cell are inside the band of a map at one sub-cell per cell only
        assert D.band_counts(board, coords, axis, 0)[0] > D.band_counts(board, coords, axis, 2)[0]
    if cell_size in (0.3, 0.1):
        assert D.quotient_crossings(board, xs, 0) + D.quotient_crossings(board, ys, 1) > 0


@pytest.mark.parametrize("cell_size", [4.0, 3.0])
def test_patch_and_edge_grids_agree_with_the_oracle(cell_size):
    """Part B's patch grids, whose exponents are not all exact by construction (the map-edge
    grids scale the information by 1 / q0^2): exp(numpy record_exponent) == the oracle's
    likelihood bit for bit at every beam end point of a sample of candidates, and the edge grids'
    probe cells keep their mean outside their own cell."""
    grids = list(D.edge_lattices(cell_size))[::6]
    grids += list(D.patch_lattices(-600.0, cell_size, "iso"))[::8] + list(D.patch_lattices(0.0, cell_size, "rank1", True))[::8]
    for lat, n_beams, _ in grids:
        ndt = O.NDT.from_cells6(*lat.grid)
        pts = lat.points(n_beams)
        ex = lat.candidate_exponents(n_beams)
        for cand in [ix * lat.n_lin + iy for ix in (0, 1, 2, 5, 8, 13) for iy in (0, 9, 31)]:
            got = np.array([ndt.likelihood_point(x, y) for x, y in pts[cand]])
            want = np.array([math.exp(e) if e > -np.inf else 0.0 for e in ex[cand]])
            assert _same_bits(got, want).all(), cand
    lat = next(D.edge_lattices(cell_size))[0]
    probe = lat.cells6[lat.size_x * 3 + 2 * 8 + 2]          # row 3, the second probe cell
    centre_x = lat.origin[0] + cell_size * (2 * 8 + 2 + 0.5)
    assert probe[5] == 5.0 and probe[0] == centre_x - cell_size and probe[2] == probe[4] > 0
