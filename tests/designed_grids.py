"""Designed cell grids: NDT grids whose cell records ARE the test vectors.

ndt2d_set_grid takes the cells6 records themselves and ndt2d_set_search the offset, cos and sin
tables themselves, so a test can put any double it likes in front of the kernels' exp(), of their
term skipping and of their cell indexing, through the public C-ABI alone.

The construction.  A cell of size c whose mean is its centre, with n = 5 and information
(-2 e, 0, 0), gives the point exactly 1.0 to the right of its mean the exponent EXACTLY e, for
any double e:  q = (1, 0), r0 = 1 * h00 + 0 * h01 = h00 = -0.5 * (-2 e) = e, r1 = 0,
exponent = r0 * 1 + r1 * 0 = e -- every operation is exact (the scalings are by powers of two).
A search whose offset table holds ascending multiples of c, around a robot that stands on a
cell's mean with theta = 0 (cos = 1 and sin = 0 given as such), and the beam (1, 0) visit one such
point per candidate; beams (1 + k c, 0) walk along a grid row, so that the row is the candidate's
list of exponents.  All coordinates are dyadic: every sum that forms a point is exact whatever
its order.

Plain module (no fixtures): builders, the high-precision reference of exp() -- the standard
library's `decimal` at 50 digits -- and numpy restatements of the kernels' record_exponent and
of NDT::getIndex.  Used by tests/test_designed_grids.py (CPU) and tests/test_gpu_designed_grids.py.
"""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

LN2 = 0.6931471805599453
# exp(x) = +inf for x above this (glibc, IEEE): csrc/ndt2d_device_fn.h kExpOverflowAbove
EXP_OVERFLOW_ABOVE = float.fromhex("0x1.62e42fefa39efp+9")
# exp(x) rounds to +0.0 for every x below this (2^-1075 = exp(-745.13321910194122...))
EXP_ZERO_BELOW = -745.14
DBL_MIN = 2.2250738585072014e-308
PREC = 50


# ---------------------------------------------------------------------------------------------
# reference of exp()
# ---------------------------------------------------------------------------------------------

def decimal_exp(x):
    """exp(x) of the exactly converted double x, 50 significant digits."""
    with localcontext() as ctx:
        ctx.prec = PREC
        return Decimal(float(x)).exp()


def _unit_exponent(y):
    """k with 2^k = ulp(y) for a normal double y > 0, = 2^-1074 for a subnormal one or 0."""
    return max(math.frexp(y)[1] - 53, -1074) if y > 0.0 else -1074


def _to_units(d, y, k):
    """(d - y) / 2^k as a float: d a Decimal, y the double nearest to it, 2^k the unit."""
    with localcontext() as ctx:
        ctx.prec = PREC
        return float((d - Decimal(y)) / (Decimal(2) ** k))


class Reference:
    """High-precision values v[i] > 0 (Decimals) prepared for vectorised error measurement:
    y = RN(v) (float(Decimal) is correctly rounded), k = the exponent of its unit -- ulp(y), or
    2^-1074 below DBL_MIN -- and v - y in those units.  A double `got` near y has got - y exact,
    so error(got) = |got - v| / unit = |(got - y) / unit - (v - y) / unit| loses nothing."""

    def __init__(self, values):
        self.values = list(values)
        self.y = np.array([float(v) for v in self.values], dtype=np.float64)
        self.k = np.array([_unit_exponent(y) for y in self.y], dtype=np.int64)
        self.resid = np.array([_to_units(v, y, int(k))
                               for v, y, k in zip(self.values, self.y, self.k)], dtype=np.float64)
        self.normal = self.y >= DBL_MIN

    def error(self, got):
        """|got - v| in units of ulp(RN(v)) (normal results) or of 2^-1074 (subnormal ones).
        inf or NaN where `got` is."""
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.abs(np.ldexp(got - self.y, -self.k) - self.resid)


def exp_reference(xs):
    """Reference of exp over finite doubles xs in [EXP_ZERO_BELOW, EXP_OVERFLOW_ABOVE]."""
    return Reference(decimal_exp(x) for x in xs)


def ulp_error(got, x):
    """|got - exp(x)| in units of ulp(RN(exp x)), for a normal result."""
    ref = exp_reference([x])
    assert ref.normal[0], x
    return float(ref.error([got])[0])


def subnormal_units(got, x):
    """|got - exp(x)| in units of 2^-1074, for a result below DBL_MIN."""
    ref = exp_reference([x])
    assert not ref.normal[0], x
    return float(ref.error([got])[0])


def decimal_sum(terms):
    with localcontext() as ctx:
        ctx.prec = PREC
        s = Decimal(0)
        for t in terms:
            s += t
        return s


# ---------------------------------------------------------------------------------------------
# the exponent vector set
# ---------------------------------------------------------------------------------------------

def _neighbours(x, n):
    """x and its n neighbouring doubles either side."""
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def exponent_vectors(seed=1):
    """About 61,000 doubles: the exponents put in front of the kernels' exp()."""
    rng = np.random.default_rng(seed)
    parts = [
        -np.exp(rng.uniform(math.log(1e-3), math.log(746.0), 20000)),   # log-uniform negative
        rng.uniform(-746.0, 0.0, 12000),
        rng.uniform(-745.2, -708.3, 6000),                              # subnormal results
        rng.uniform(0.0, 709.79, 6000),                                 # negative definite information
    ]
    special = []
    for k in range(-1076, 1025):
        special += _neighbours((k + 0.5) * LN2, 2)      # rint ties of n = rint(x log2 e)
        special += _neighbours(k * LN2, 1)
    special += _neighbours(EXP_OVERFLOW_ABOVE, 1) + [710.0, 1000.0, 1e15, 1e300, np.inf]
    special += [-745.1332191019411, -745.1332191019412, -745.2, -746.0]
    special += _neighbours(-1000.0, 1) + [-1e300, -np.inf]
    for v in (0.0, 2.0 ** -54, 2.0 ** -53, 1e-300, 5e-324):
        special += [v, -v]
    special += [np.nan]
    return np.concatenate(parts + [np.array(special, dtype=np.float64)])


def classify(e):
    """Masks over exponents: (referenced, zero, inf, nan).  `referenced`: finite, in
    [EXP_ZERO_BELOW, EXP_OVERFLOW_ABOVE] -- compared with the decimal reference; `zero`: below
    EXP_ZERO_BELOW -- exactly +0.0; `inf`: above EXP_OVERFLOW_ABOVE -- exactly +inf."""
    e = np.asarray(e, dtype=np.float64)
    nan = np.isnan(e)
    with np.errstate(invalid="ignore"):
        zero = e < EXP_ZERO_BELOW
        inf = e > EXP_OVERFLOW_ABOVE
    return ~(nan | zero | inf), zero, inf, nan


# ---------------------------------------------------------------------------------------------
# numpy restatements of the kernels' arithmetic (plain float64 operations, no fused multiply-add)
# ---------------------------------------------------------------------------------------------

def record_exponent(cells6, px, py):
    """csrc/ndt2d_device_fn.h record_exponent on records given as cells6 rows, in its operation
    order: h = -0.5 * information, r = q h, exponent = r0 q0 + r1 q1."""
    c = np.asarray(cells6, dtype=np.float64).reshape(-1, 6)
    with np.errstate(invalid="ignore", over="ignore"):
        h00, h01, h11 = -0.5 * c[:, 2], -0.5 * c[:, 3], -0.5 * c[:, 4]
        q0 = px - c[:, 0]
        q1 = py - c[:, 1]
        r0 = q0 * h00 + q1 * h01
        r1 = q0 * h01 + q1 * h11
        return r0 * q0 + r1 * q1


def get_index(x, y, size_x, size_y, cell_size, origin):
    """NDT::getIndex: int((x - o) / c) after the `x < o` test; -1 outside the grid."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    fx = (x - origin[0]) / cell_size
    fy = (y - origin[1]) / cell_size
    inside = (x >= origin[0]) & (y >= origin[1]) & (fx < size_x) & (fy < size_y)
    gx = np.where(inside, fx, 0.0).astype(np.int64)
    gy = np.where(inside, fy, 0.0).astype(np.int64)
    return np.where(inside, gy * size_x + gx, -1)


def kernel_negligible_below(s):
    """csrc/ndt2d_device_fn.h negligible_below(s): fma(frexp_exponent(s) - 1, ln 2, -38) (one
    rounding, taken here through exact rational arithmetic), floored at -746."""
    if not s > 0.0:
        return -746.0
    k = math.frexp(s)[1] - 1
    v = float(Fraction(k) * Fraction(LN2) - 38)
    return v if v > -746.0 else -746.0


# ---------------------------------------------------------------------------------------------
# grids and the searches that visit them
# ---------------------------------------------------------------------------------------------

def records_for(e, mean_x, mean_y, shape):
    """cells6 records that give the point mean + (1, 0) the exponent e.  shape "rank1":
    information (-2 e, 0, 0), for which the occupancy map makes no claim (every term takes the
    exact path); "iso": (-2 e, 0, -2 e), e < 0, for which sub-cell bounds are claimed."""
    e = np.asarray(e, dtype=np.float64)
    rec = np.zeros((len(e), 6))
    rec[:, 0] = mean_x
    rec[:, 1] = mean_y
    rec[:, 2] = -2.0 * e
    if shape == "iso":
        assert np.all(e < 0.0) and np.all(np.isfinite(e))
        rec[:, 4] = -2.0 * e
    else:
        assert shape == "rank1", shape
    rec[:, 5] = 5.0
    return rec


class Lattice:
    """A designed grid together with the search that visits it.

    E[gy, gx]: the exponent cell (gx, gy) gives the point 1.0 to the right of its mean; cells
    where `occupied` is False are empty (n = 0).  The grid's origin is (-c h, -c h), h =
    n_lin // 2, so that cell (h, h) has its mean at (c / 2, c / 2): there the robot stands, with
    theta = 0, and the offsets are dlin[i] = c (i - h).  Candidate (ix, iy) -- flat index
    ix * n_lin + iy -- stands on the mean of cell (ix, iy); its beam k = (1 + k c, 0) ends 1.0 to
    the right of the mean of cell (ix + k, iy), or off the grid."""

    def __init__(self, E, cell_size, shape="rank1", n_lin=None, occupied=None, n_points=5.0,
                 stride=1, beam_x=1.0, mean_dx=None):
        """stride, beam_x, mean_dx (part B's edge grids): beam k ends beam_x to the right of the
        CENTRE of cell (ix + stride k, iy), and cell (gx, gy) has its mean mean_dx[gy, gx] to the
        right of its centre (default: beam_x - 1, i.e. the point is mean + (1, 0) as above).  Where
        the point is not mean + (1, 0) the information is -2 e / q0^2, which rounds: E then holds
        the exponent the numpy record_exponent gives, in place of the intended one."""
        E = np.array(E, dtype=np.float64)
        self.E = E
        self.stride, self.beam_x = int(stride), float(beam_x)
        self.size_y, self.size_x = E.shape
        self.cell_size = float(cell_size)
        self.n_lin = int(n_lin if n_lin is not None else max(E.shape))
        self.occupied = np.ones(E.shape, bool) if occupied is None else np.asarray(occupied, bool)
        c, h = self.cell_size, self.n_lin // 2
        assert c * 0.5 == math.floor(c * 0.5 * 2) / 2 and c >= 3.0     # means are dyadic, 1 / c < 1 / 2
        self.origin = (-c * h, -c * h)
        self.pose = (c / 2, c / 2)
        self.dlin = c * (np.arange(self.n_lin, dtype=np.float64) - h)
        gy, gx = np.divmod(np.arange(E.size), self.size_x)
        centre_x = self.origin[0] + c * (gx + 0.5)
        mean_dx = np.full(E.size, self.beam_x - 1.0) if mean_dx is None else np.asarray(mean_dx, dtype=np.float64).ravel()
        mean_x = centre_x + mean_dx
        mean_y = self.origin[1] + c * (gy + 0.5)
        q0 = (centre_x + self.beam_x) - mean_x
        flat_e = E.ravel()
        occ = self.occupied.ravel()
        rec = np.zeros((E.size, 6))
        scaled = np.where(q0 == 1.0, flat_e, flat_e / (q0 * q0))
        rec[occ] = records_for(scaled[occ], mean_x[occ], mean_y[occ], shape)
        rec[occ, 5] = n_points
        self.cells6 = rec
        off = occ & (q0 != 1.0)
        if off.any():
            flat_e[off] = record_exponent(rec[off], (centre_x + self.beam_x)[off], mean_y[off])

    @property
    def grid(self):
        """(cells6, size_x, size_y, cell_size, origin)"""
        return self.cells6, self.size_x, self.size_y, self.cell_size, self.origin

    def beams(self, n_beams):
        b = np.zeros((n_beams, 2))
        b[:, 0] = self.beam_x + self.stride * self.cell_size * np.arange(n_beams)
        return b

    def poses(self):
        """The pose of every candidate, flat order: the same points through the particle path."""
        ix, iy = np.divmod(np.arange(self.n_lin ** 2), self.n_lin)
        return np.column_stack([self.pose[0] + self.dlin[ix], self.pose[1] + self.dlin[iy],
                                np.zeros(len(ix))])

    def candidate_exponents(self, n_beams):
        """[n_lin^2, n_beams]: the intended exponent of every (candidate, beam); -inf (a term
        of +0.0) where the beam ends in an empty cell or off the grid."""
        ix, iy = np.divmod(np.arange(self.n_lin ** 2), self.n_lin)
        out = np.full((len(ix), n_beams), -np.inf)
        for k in range(n_beams):
            gx = ix + self.stride * k
            ok = (gx < self.size_x) & (iy < self.size_y)
            ok[ok] = self.occupied[iy[ok], gx[ok]]
            out[ok, k] = self.E[iy[ok], gx[ok]]
        return out

    def points(self, n_beams):
        """[n_lin^2, n_beams, 2]: the beam end points, formed as the kernels form them
        ((bx * cos - by * sin + pose_x) + dx with cos = 1, sin = 0: all exact)."""
        ix, iy = np.divmod(np.arange(self.n_lin ** 2), self.n_lin)
        b = self.beams(n_beams)
        px = (b[None, :, 0] + self.pose[0]) + self.dlin[ix][:, None]
        py = (b[None, :, 1] + self.pose[1]) + self.dlin[iy][:, None]
        return np.stack([px, py], axis=-1)


def vector_chunks(vectors, side, cell_size, shape="rank1"):
    """The vectors cut into side x side grids, one vector per cell (vector j of a chunk in cell
    j = gy * side + gx), searched with one beam.  Yields (lattice, vector index of every
    candidate [side^2], -1 where the chunk's last grid has no vector)."""
    vectors = np.asarray(vectors, dtype=np.float64)
    per = side * side
    for at in range(0, len(vectors), per):
        part = vectors[at:at + per]
        E = np.zeros(per)
        E[:len(part)] = part
        occ = np.arange(per) < len(part)
        if shape == "iso":
            E[len(part):] = -1.0
        lat = Lattice(E.reshape(side, side), cell_size, shape, side, occ.reshape(side, side))
        ix, iy = np.divmod(np.arange(per), side)
        cell = iy * side + ix
        yield lat, np.where(cell < len(part), at + cell, -1)


# ---------------------------------------------------------------------------------------------
# part A, sums: candidates whose terms span 300 orders of magnitude
# ---------------------------------------------------------------------------------------------

def sum_lattice(cell_size, n_rows=8, n_beams=256, seed=11, shape="rank1"):
    """n_rows rows of n_rows + n_beams cells: candidate (ix, iy) sums the n_beams cells from ix
    on of row iy (2,112 cells by default: the records still fit LDS).  Rows 0 .. n_rows - 5: exponents uniform over 300 orders of magnitude; the next
    two: all-tiny (every term below 1e-140); the last two: a few large terms in a sea of tiny ones."""
    rng = np.random.default_rng(seed)
    w = n_rows + n_beams
    E = np.zeros((n_rows, w))
    for r in range(n_rows):
        if r < n_rows - 4:
            E[r] = rng.uniform(-690.0, -1e-3, w)
        elif r < n_rows - 2:
            E[r] = rng.uniform(-740.0, -323.0, w)
        else:
            E[r] = rng.uniform(-740.0, -323.0, w)
            E[r, rng.choice(w, 12, replace=False)] = rng.uniform(-3.0, -1e-3, 12)
    return Lattice(E, cell_size, shape, n_rows)


# ---------------------------------------------------------------------------------------------
# part B: skipping at its boundaries
# ---------------------------------------------------------------------------------------------

def skip_carriers():
    """name -> (list of carrier exponents, needs positive exponents).  The carriers' terms make
    the running sum s: exactly 2^k (k cells of exponent 0), one ulp either side of 1
    (e = +-2^-53: exp = 1 + 2^-52 and 1 - 2^-53 after rounding), tiny, subnormal."""
    return {
        "1": [0.0], "2": [0.0] * 2, "4": [0.0] * 4, "8": [0.0] * 8,
        "1+ulp": [2.0 ** -53], "1-ulp": [-2.0 ** -53],
        "tiny": [-600.0], "subnormal": [-740.0],
    }


def carrier_sum(exps):
    """The running sum the carriers make, in double arithmetic with correctly rounded terms."""
    s = 0.0
    for e in exps:
        s += float(decimal_exp(e))
    return s


def skip_probes(s):
    """Probe exponents for a running sum s: a sweep of +-2 around T(s) = ln s - 54 ln 2 (a term
    of 2^-54 s: half an ulp of a sum just below a power of two), and the eight doubles either side
    of the kernel's own bound, of T(s) and of T(s) + ln 2 (half an ulp of a sum s = 2^k)."""
    t = math.log(s) - 54.0 * LN2
    out = list(t + np.linspace(-2.0, 2.0, 41))
    for centre in (kernel_negligible_below(s), t, t + LN2):
        out += _neighbours(centre, 8)
    out = np.array(out)
    return out[(out < -1e-9) & (out > -1.0e3)]


def skip_rows(shape):
    """[(row of exponents, name of the carrier, index of the probe in the row)]: carriers first
    and probe first.  shape "iso" leaves out the carrier that needs a positive exponent and
    takes the exponent 0 as -2^-60 (exp = 1 - 2^-60 -> 1.0 after rounding: the same sums)."""
    rows = []
    for name, carriers in skip_carriers().items():
        if shape == "iso":
            if name == "1+ulp":
                continue
            carriers = [e if e < 0.0 else -2.0 ** -60 for e in carriers]
        rows.append((list(carriers), name, -1))
        for p in skip_probes(carrier_sum(carriers)):
            rows.append((list(carriers) + [float(p)], name, len(carriers)))
            rows.append(([float(p)] + list(carriers), name, 0))
    return rows


def level_rows():
    """Isotropic cells whose exponent at the probe point lies within 1e-6 (and 1e-9) either side
    of every integer from -62 to -1 -- the levels of map_byte and skip_level -- behind carriers
    that put the skip threshold next to that integer ([carrier, probe] and [probe, carrier] with
    ln(carrier sum) ~ e + 38, where such a sum exists), and behind a sum of 1.  (A cell whose mean
    lies inside it has its own mean in its map box, so its byte claims nothing and these terms
    meet the exponent compare `e < skip_below` at the integers, not the byte compare.)"""
    rows = []
    for j in range(1, 63):
        for d in (-1e-6, -1e-9, 0.0, 1e-9, 1e-6):
            p = -float(j) + d
            # negligible_below(s) = (frexp_exp(s) - 1) ln 2 - 38 ~ p  <=>  ln s ~ p + 38
            for carrier in (-2.0 ** -60, min(p + 38.0, -2.0 ** -60), min(p + 38.5, -2.0 ** -60)):
                rows.append(([carrier, p], "level", 1))
                rows.append(([p, carrier], "level", 0))
    return rows


def rows_lattices(rows, cell_size, shape, n_lin=32):
    """The rows packed n_lin to a grid (row r of a chunk = grid row r; cells behind a row's end
    are empty).  Yields (lattice, rows of the chunk, n_beams)."""
    for at in range(0, len(rows), n_lin):
        part = rows[at:at + n_lin]
        width = max(max(len(r[0]) for r in part), n_lin)
        E = np.full((n_lin, width), -1.0)
        occ = np.zeros((n_lin, width), bool)
        for r, (exps, _, _) in enumerate(part):
            E[r, :len(exps)] = exps
            occ[r, :len(exps)] = True
        yield Lattice(E, cell_size, shape, n_lin, occ), part, max(len(r[0]) for r in part)


def patch_carriers(shape):
    """name -> exponent of the carrier cells of a patch lattice (see patch_lattices)."""
    out = {"1": 0.0, "1+ulp": 2.0 ** -53, "1-ulp": -2.0 ** -53, "tiny": -600.0, "subnormal": -740.0}
    if shape == "iso":
        del out["1+ulp"]
        out["1"] = -2.0 ** -60       # exp = 1 - 2^-60 -> 1.0 after rounding
    return out


def patch_probes(carrier_e, n_carriers=8):
    """Probe exponents for running sums s = m exp(carrier_e), m = 1 .. n_carriers: the eight
    doubles either side of the kernel's own bound for every such sum, and a sweep from 2.25 below
    to 4.25 above T = ln s_1 - 54 ln 2 (the half-ulp thresholds of all the sums lie inside it)."""
    t1 = float(decimal_exp(carrier_e))
    out = []
    s = 0.0
    for _ in range(n_carriers):
        s += t1
        out += _neighbours(kernel_negligible_below(s), 8)
    out += list(math.log(t1) - 54.0 * LN2 + np.arange(-2.25, 4.26, 0.25))
    out += list(np.arange(-747.0, -739.0, 0.25)) if carrier_e < -700.0 else []
    out = np.unique(np.array(out))
    return out[(out < -1e-9) & (out > -1.0e3)]


def patch_lattices(carrier_e, cell_size, shape, probe_first=False, n_lin=32, n_carriers=8, n_beams=24):
    """Grids on which the lane kernels' skipping is what decides the result.  A lane kernel gives
    up a term only when NONE of the 64 candidates of a patch (8 x 8 translations, one wave) needs
    it, against a threshold taken from the lane's sum after the previous group of eight beams.
    So every row holds n_carriers carrier cells and then n_beams probe cells of ONE exponent, the
    same over the eight rows of a patch: candidate (ix, iy), ix < 8, meets 8 - ix carriers in its
    first group of beams and nothing but probes from then on, and so do all its patch mates --
    running sums of 1 .. 8 carriers side by side in one wave.  probe_first: the probes, then the
    carriers.  Yields (lattice, n_beams, the probe of every row block [n_lin / 8])."""
    probes = patch_probes(carrier_e, n_carriers)
    blocks = n_lin // 8
    width = n_lin + n_beams
    for at in range(0, len(probes), blocks):
        part = probes[at:at + blocks]
        part = np.concatenate([part, np.full(blocks - len(part), part[-1])])
        E = np.repeat(part, 8)[:, None] * np.ones((1, width))
        if probe_first:
            E[:, n_beams - n_carriers:n_beams] = carrier_e
        else:
            E[:, :n_carriers] = carrier_e
        yield Lattice(E, cell_size, shape, n_lin), n_beams, part


def edge_lattices(cell_size, n_lin=32, n_carriers=8, n_beams=24):
    """Patch grids (see patch_lattices) on which the occupancy map's byte is what gives a term
    up.  Beams step two cells, so that a probe cell's neighbours along the row are empty, and end
    c / 512 inside the cell's left edge; a probe cell is isotropic with its mean a whole cell to the
    left of its centre: its map box (the cell, widened by c / 1024) does not hold the mean, and the
    bound the byte claims, h (c / 2 - c / 1024)^2 + slack, lies 1.2 % above the exponent the point
    really gets, h (c / 2 + c / 512)^2.  The information sweeps that bound across the integers
    -46 .. -30 (the levels of map_byte that running sums of 1 .. 8 compare with) and their
    neighbourhoods.  Yields (lattice, n_beams, the bound aimed at for every row block)."""
    c = float(cell_size)
    beam_x = -c / 2 + c / 512
    q_box = c / 2 - c / 1024
    q_pt = c / 2 + c / 512
    aims = []
    for j in range(-46, -29):
        aims += [j - 0.5, j - 1e-3, j - 3e-6, j - 1e-6, float(j), j + 1e-6, j + 1e-3]
    aims = np.array(aims)
    blocks = n_lin // 8
    width = n_lin + 2 * n_beams
    for at in range(0, len(aims), blocks):
        part = aims[at:at + blocks]
        part = np.concatenate([part, np.full(blocks - len(part), part[-1])])
        h = np.repeat(part, 8) / (q_box * q_box)
        E = (h * (q_pt * q_pt))[:, None] * np.ones((1, width))
        mean_dx = np.full(E.shape, -c)
        occ = np.zeros(E.shape, bool)
        occ[:, ::2] = True
        E[:, :2 * n_carriers] = -2.0 ** -60
        mean_dx[:, :2 * n_carriers] = beam_x - 1.0
        yield Lattice(E, c, "iso", n_lin, occ, stride=2, beam_x=beam_x, mean_dx=mean_dx), n_beams, part


def long_rows_lattice(cell_size, shape, n_rows=8, n_beams=320, seed=5):
    """Candidates of more than 64 beams and of more than any one wave's share of a block: a
    carrier of 1.0 first, last or in the middle, probes at the skip threshold and tiny terms
    around it, so that several waves each hold a partial sum."""
    rng = np.random.default_rng(seed)
    w = n_rows + n_beams
    zero = -2.0 ** -60 if shape == "iso" else 0.0
    t = -54.0 * LN2
    E = rng.uniform(t - 2.0, t + 2.0, (n_rows, w))
    E[:, ::7] = rng.uniform(-700.0, -100.0, E[:, ::7].shape)
    for r in range(n_rows):
        E[r, (0, w - 1, w // 2, 65, 5, 130, 200, 258)[r % 8]] = zero
    return Lattice(E, cell_size, shape, n_rows)


# ---------------------------------------------------------------------------------------------
# part C: cell choice made visible
# ---------------------------------------------------------------------------------------------

class Checkerboard:
    """size x size cells on which any wrong cell is a gross error: neighbours along either axis
    alternate between a cell of zero information (term exp(0) = 1.0 wherever the point lies in
    it) and one whose mean lies 1,000 m to its left with information (6e-5, 0, 0) (term about
    exp(-30) = 9e-14 anywhere in the cell); some cells are empty, some have n = 4 (neither can
    score); the rightmost column and the top row are all of the first kind."""

    def __init__(self, cell_size, origin, size=10, seed=3):
        rng = np.random.default_rng(seed)
        self.size_x = self.size_y = size
        self.cell_size = float(cell_size)
        self.origin = (float(origin[0]), float(origin[1]))
        gy, gx = np.divmod(np.arange(size * size), size)
        cx = self.origin[0] + self.cell_size * (gx + 0.5)
        cy = self.origin[1] + self.cell_size * (gy + 0.5)
        rec = np.zeros((size * size, 6))
        ones = ((gx + gy) % 2 == 0) | (gx == size - 1) | (gy == size - 1)
        rec[:, 0] = np.where(ones, cx, cx - 1000.0)
        rec[:, 1] = cy
        rec[:, 2] = np.where(ones, 0.0, 6e-5)
        rec[:, 5] = 5.0
        interior = (gx < size - 1) & (gy < size - 1)
        pick = rng.choice(np.flatnonzero(interior), size * size // 6, replace=False)
        rec[pick[::2], 5] = 0.0
        rec[pick[1::2], 5] = 4.0
        self.cells6 = rec
        self.kind = np.where(rec[:, 5] < 5.0, 0, np.where(ones, 1, 2))   # 0: no term, 1: 1.0, 2: exp(-30)

    @property
    def grid(self):
        return self.cells6, self.size_x, self.size_y, self.cell_size, self.origin

    def expected_terms(self, px, py):
        """The term of every point (px[i], py[i]): the cell by getIndex, the record's likelihood
        (1.0, about 9e-14, or 0.0 for a cell that cannot score or a point off the grid)."""
        idx = get_index(px, py, self.size_x, self.size_y, self.cell_size, self.origin)
        rec = self.cells6[np.maximum(idx, 0)]
        term = np.exp(record_exponent(rec, np.asarray(px), np.asarray(py)))
        return np.where((idx >= 0) & (rec[:, 5] >= 5.0), term, 0.0)

    def boundaries(self, axis):
        """The doubles o + k c, k = 0 .. size: the origin, every interior boundary, the far edge."""
        return self.origin[axis] + self.cell_size * np.arange(self.size_x + 1, dtype=np.float64)

    def coordinates(self, axis):
        """Probe coordinates along one axis, ascending: every boundary o + k c itself and its
        four neighbouring doubles either side (which hold the points whose quotient (x - o) / c
        rounds across an integer), points 1/4 .. 64 units of 2^-16 cell below and above it (few enough for
        the union of both axes' coordinates to stay a lattice the small-lattice search takes) (the
        lane kernels' guard band is kNearUnits = 4 units of 2^-16 map sub-cell either side of a
        boundary, 1 .. 4 sub-cells per cell: see band_counts), and the middle
        of every cell, of the cell before the origin and of the one behind the far edge."""
        c = self.cell_size
        out = []
        for b in self.boundaries(axis):
            out += _neighbours(b, 4)
            for u in (0.25, 0.75, 1, 3, 4, 5, 8, 16, 64):
                out += [b - u * c / 65536.0, b + u * c / 65536.0]
            out += [b - 0.5 * c, b + 0.5 * c]
        return np.unique(np.array(out, dtype=np.float64))


def band_counts(board, xs, axis, sub_log2=0):
    """The lane kernels' guard band (csrc/ndt2d_lane_fn.h: kNearUnits, near_boundary): a point
    whose 16-bit fraction of a map sub-cell, biased by 4, is below 8 -- within 4 units of 2^-16
    SUB-cell below a sub-cell boundary or less than 4 above it -- takes the reference's own index
    arithmetic.  The map holds 2^sub_log2 sub-cells per cell (0 for the small-lattice search, up
    to 2 for the large one; a launch does not report which), so a unit is 2^-(16 + sub_log2) cell.
    Of the coordinates inside the grid, how many lie in that band around a CELL boundary, and how
    many just outside it (beyond the band, within 64 units of a cell boundary): (inside, outside)."""
    f = (np.asarray(xs) - board.origin[axis]) / board.cell_size
    ok = (f > 0.0) & (f < board.size_x)
    units = 65536.0 * (1 << sub_log2)
    below = (np.ceil(f) - f) * units       # units up to the next cell boundary
    above = (f - np.floor(f)) * units      # units from the last one
    inside = ok & (((below > 0.0) & (below <= 4.0)) | (above < 4.0))
    outside = ok & ~inside & ((below <= 64.0) | (above <= 64.0))
    return int(inside.sum()), int(outside.sum())


def quotient_crossings(board, xs, axis):
    """Coordinates whose double quotient (x - o) / c truncates to another integer than the exact
    quotient of the same doubles does (0.3 / 0.1 = 2.9999999999999996 is such a quotient)."""
    o, c = board.origin[axis], board.cell_size
    n = 0
    for x in np.asarray(xs):
        if not x >= o:
            continue
        exact = math.floor((Fraction(float(x)) - Fraction(o)) / Fraction(c))
        if int((float(x) - o) / c) != exact:
            n += 1
    return n


def rotated_origin(beam, cos_t, sin_t):
    """(A, B) = the rotated beam in the kernels' operation order, bx * cos - by * sin and
    bx * sin + by * cos: a robot at (-A, -B) puts that beam's end exactly on (0, 0), so that the
    offsets themselves are the points."""
    a = beam[0] * cos_t - beam[1] * sin_t
    b = beam[0] * sin_t + beam[1] * cos_t
    return a, b


def search_points(beam, pose, cos_t, sin_t, dlin):
    """The points of a search of one beam in the kernels' operation order,
    (bx * cos - by * sin + pose_x) + dx: (x[n_lin], y[n_lin]); candidate (ix, iy) is at (x[ix], y[iy])."""
    a, b = rotated_origin(beam, cos_t, sin_t)
    return (a + pose[0]) + dlin, (b + pose[1]) + dlin
