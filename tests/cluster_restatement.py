"""The particle clusterer (include/ndt2d_hip.h, "Pose clusters"; csrc/cluster/) restated on the CPU in
numpy and Python integers.  Test infrastructure only: nothing of the product is imported.  The
yardstick of tests/test_cluster_restatement.py (which pins it to cases worked by hand) and of
tests/test_gpu_clusters.py.

    kx = floor(x / cell_x), ky = floor(y / cell_y)
    t  = theta into [-pi, pi): r = fmod(theta, 2 pi); r += 2 pi where r < -pi; r -= 2 pi where r >= pi
    kt = min(n_theta - 1, trunc((t + pi) / (2 pi) * n_theta))
    left out: a pose that is not finite, |x / cell| or |y / cell| >= 2^30, a weight not in [0, 1]
    components of the occupied bins under the 26-neighbourhood, kt modulo n_theta, by union-find;
    a component's label is its smallest particle index
    q = trunc(w 2^40) as a Python integer, Q their sum; rank: Q descending, label ascending
    statistics of the first max_clusters: math.fsum of the terms, and beside each the sum of the
    absolute terms (what a bound on a summation tree is stated in)
Every key step is float64 arithmetic that IEEE fixes to the bit.
"""
import math

import numpy as np

PI = np.float64(np.pi)
TWO_PI = np.float64(2.0) * PI
KEY_LIMIT = np.float64(2.0 ** 30)
TWO40 = np.float64(2.0 ** 40)
LEFT_OUT = 0xffffffff


def normalise_angle(theta):
    with np.errstate(invalid="ignore"):
        r = np.fmod(np.asarray(theta, dtype=np.float64), TWO_PI)
        r = np.where(r < -PI, r + TWO_PI, r)
        r = np.where(r >= PI, r - TWO_PI, r)
    return r


def theta_bin(t, n_theta):
    scaled = (np.asarray(t, dtype=np.float64) + PI) / TWO_PI * np.float64(n_theta)
    return np.minimum(n_theta - 1, np.trunc(scaled).astype(np.int64))


def uniform_weights(n):
    return np.full(n, np.float64(1.0) / np.float64(n)) if n else np.zeros(0)


def keys(poses, weights, cell_x=0.5, cell_y=0.5, n_theta=24):
    """(kx, ky, kt) as int64 arrays and the left-out mask; the keys of left-out particles are 0, 0, -1."""
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    w = uniform_weights(len(p)) if weights is None else np.asarray(weights, dtype=np.float64)
    with np.errstate(all="ignore"):
        qx = p[:, 0] / np.float64(cell_x)
        qy = p[:, 1] / np.float64(cell_y)
        ok = np.isfinite(p).all(axis=1) & (w >= 0.0) & (w <= 1.0)
        ok &= (np.abs(qx) < KEY_LIMIT) & (np.abs(qy) < KEY_LIMIT)
        kx = np.where(ok, np.floor(np.where(ok, qx, 0.0)), 0.0).astype(np.int64)
        ky = np.where(ok, np.floor(np.where(ok, qy, 0.0)), 0.0).astype(np.int64)
        kt = np.where(ok, theta_bin(normalise_angle(np.where(ok, p[:, 2], 0.0)), n_theta), -1).astype(np.int64)
    return kx, ky, kt, ~ok


def mass_q(w):
    """trunc(w 2^40) of one weight in [0, 1], a Python integer (the product is exact)."""
    return int(float(np.float64(w) * TWO40))


def key_hash(kx, ky, kt):
    return ((kx & 0xffffffff) * 0x9E3779B1 + (ky & 0xffffffff) * 0x85EBCA77 + (kt & 0xffffffff) * 0xC2B2AE3D) & 0xffffffff


def neighbours(key, n_theta):
    """The 26 neighbour keys in the header's order: dt slowest, dx fastest, (0, 0, 0) skipped."""
    kx, ky, kt = key
    out = []
    for dt in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dt) != (0, 0, 0):
                    out.append((kx + dx, ky + dy, (kt + dt) % n_theta))
    return out


def ranks_before(q_a, label_a, q_b, label_b):
    return q_a > q_b or (q_a == q_b and label_a < label_b)


def _fsum_abs(terms):
    return math.fsum(terms), math.fsum(abs(v) for v in terms)


def centred_moments(poses, weights, members, W, mx, my, mt):
    """({cxx, cxy, cyy, vt}, {xx, xy, yy, tt}) of the particles `members` round the centre (mx, my,
    mt): math.fsum of w dx dx, w dx dy, w dy dy and w d d over W, d = theta - mt normalised, and the
    sums of the absolute terms.  cluster() calls it with the cluster's own means; a test of a
    two-pass implementation calls it again with the means that implementation reports (which it
    holds to the fsum means separately), so that the second pass is held to the bound of ITS sums:
    a centred term of a cluster that is narrower than the rounding of its mean has no other yardstick."""
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ww = np.asarray(weights, dtype=np.float64)[members]
    with np.errstate(all="ignore"):
        dx, dy = p[members, 0] - np.float64(mx), p[members, 1] - np.float64(my)
        d = normalise_angle(p[members, 2] - np.float64(mt))
        out, out_abs = {}, {}
        for name, short, terms in (("cxx", "xx", ww * dx * dx), ("cxy", "xy", ww * dx * dy), ("cyy", "yy", ww * dy * dy),
                                   ("vt", "tt", ww * d * d)):
            total, out_abs[short] = _fsum_abs(terms.tolist())
            out[name] = float(np.float64(total) / np.float64(W))
    return out, out_abs


def cluster(poses, weights, cell_x=0.5, cell_y=0.5, n_theta=24, max_clusters=8):
    """Returns {"labels": uint32 [n], "header": {...}, "records": [...], "poses", "weights"}; a record
    holds label, count, Q (integer), W, mx, my, mt, cxx, cxy, cyy, vt, `resultant` (the length of
    the heading's resultant over W), `members` (its particle indices) and "abs": the sums of
    absolute terms behind W, x, y, sin, cos, xx, xy, yy, tt."""
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    w = uniform_weights(n) if weights is None else np.asarray(weights, dtype=np.float64)
    kx, ky, kt, out = keys(p, weights, cell_x, cell_y, n_theta)
    labels = np.full(n, LEFT_OUT, dtype=np.uint32)
    bins = {}            # key -> its particles, ascending
    for i in np.flatnonzero(~out).tolist():
        bins.setdefault((int(kx[i]), int(ky[i]), int(kt[i])), []).append(i)
    parent = {k: k for k in bins}

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    for k in bins:
        for other in neighbours(k, n_theta):
            if other in bins:
                a, b = find(k), find(other)
                if a != b:
                    parent[a] = b
    members = {}
    for k, idx in bins.items():
        members.setdefault(find(k), []).extend(idx)
    found = []
    for idx in members.values():
        idx = np.array(sorted(idx), dtype=np.int64)
        labels[idx] = idx[0]
        found.append((sum(mass_q(v) for v in w[idx].tolist()), int(idx[0]), idx))
    found.sort(key=lambda c: (-c[0], c[1]))
    records = []
    for q, label, idx in found[:max_clusters]:
        ww, xx, yy, th = w[idx], p[idx, 0], p[idx, 1], p[idx, 2]
        W, W_abs = _fsum_abs(ww.tolist())
        sx, sx_abs = _fsum_abs((ww * xx).tolist())
        sy, sy_abs = _fsum_abs((ww * yy).tolist())
        ss, ss_abs = _fsum_abs((ww * np.sin(th)).tolist())
        sc, sc_abs = _fsum_abs((ww * np.cos(th)).tolist())
        with np.errstate(all="ignore"):
            mx, my, mt = float(np.float64(sx) / np.float64(W)), float(np.float64(sy) / np.float64(W)), math.atan2(ss, sc)
            record = {"label": label, "count": len(idx), "Q": q, "W": W, "mx": mx, "my": my, "mt": mt,
                      "resultant": float(np.float64(math.hypot(ss, sc)) / np.float64(W)), "members": idx,
                      "abs": {"W": W_abs, "x": sx_abs, "y": sy_abs, "sin": ss_abs, "cos": sc_abs}}
        moments, moments_abs = centred_moments(p, w, idx, W, mx, my, mt)
        record.update(moments)
        record["abs"].update(moments_abs)
        records.append(record)
    header = {"n": n, "n_left_out": int(out.sum()), "n_bins": len(bins), "n_clusters": len(found),
              "w_total": math.fsum(w[~out].tolist())}
    return {"labels": labels, "header": header, "records": records, "poses": p, "weights": w}
