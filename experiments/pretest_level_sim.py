#!/usr/bin/env python3
"""CPU model of the large lane search's look-up and skip logic at cfg-2, to estimate what a pre-test
against the wave's lowest skip level prunes (profiles/pretest_level_ab.json).
No GPU: the grid comes from the oracle (tests/oracle_lib.py), the scans from synth's host generator.

Restated in numpy from csrc/ndt2d_lane_fn.h and csrc/ndt2d_match_lane.hip: the map bytes of the
window at 4 x 4 sub-cells per cell with the closed-form exponent_upper_bound, the packed fixed-point
coordinates, the 64-beam pre-test over the 4 x 4 box of the patch's first lane, the groups of eight
beams, the per-lane live test against skip_level, the near-boundary band, negligible_below and the
refresh after a group that added a term.  (Not restated: exp_of_exponent's last bits -- numpy's exp
stands in -- and the reference's index arithmetic of a near lane, which picks the same cell except
on a boundary itself.)

Sample: every 8th theta step, the 144 whole 8 x 8 patches of the 100 x 100 lattice: 3,600 items.

    python3 experiments/pretest_level_sim.py [theta stride, default 8]
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
from ndt_2d_amd import synth  # noqa: E402

CFG = 2
SUB_LOG2 = 2
SUB = 1 << SUB_LOG2
BOX_MARGIN = 1.0 / 1024.0
NEAR_UNITS = 4
LN2 = 0.6931471805599453


def exponent_upper_bound(rec, x0, x1, y0, y1):
    """csrc/ndt2d_lane_fn.h exponent_upper_bound, vectorised over boxes; rec = (mx, my, h00, h01, h11)."""
    mx, my, h00, h01, h11 = rec
    ok = (h00 < 0.0) & (h11 < 0.0) & (h00 * h11 - h01 * h01 > 0.0)
    a0, a1, b0, b1 = x0 - mx, x1 - mx, y0 - my, y1 - my
    inside = (a0 <= 0.0) & (a1 >= 0.0) & (b0 <= 0.0) & (b1 >= 0.0)
    best = np.full(np.shape(a0), -np.inf)
    with np.errstate(all="ignore"):
        for q0 in (a0, a1):
            q1 = np.minimum(np.maximum(-h01 * q0 / h11, b0), b1)
            best = np.maximum(best, h00 * q0 * q0 + 2.0 * h01 * q0 * q1 + h11 * q1 * q1)
        for q1 in (b0, b1):
            q0 = np.minimum(np.maximum(-h01 * q1 / h00, a0), a1)
            best = np.maximum(best, h00 * q0 * q0 + 2.0 * h01 * q0 * q1 + h11 * q1 * q1)
    best = np.where(inside, 0.0, best)
    am, bm = np.maximum(np.abs(a0), np.abs(a1)), np.maximum(np.abs(b0), np.abs(b1))
    mag = np.abs(h00) * am * am + 2.0 * np.abs(h01) * am * bm + np.abs(h11) * bm * bm
    return np.where(ok, best + (1e-9 * mag + 1e-6), np.inf)


def map_levels(cells6, sx, sy, c, origin, pad, w_cells, h_cells):
    """(level [rows, cols], occupied [rows, cols]) of the window's map: sub_cell_byte + map_byte."""
    rows, cols = h_cells * SUB, w_cells * SUB
    my, mx = np.divmod(np.arange(rows * cols), cols)
    cx, cy = (mx >> SUB_LOG2) - pad, (my >> SUB_LOG2) - pad
    lx, ly = mx & (SUB - 1), my & (SUB - 1)
    sub_size = c / SUB
    x0 = origin[0] + (cx * SUB + lx - BOX_MARGIN) * sub_size
    y0 = origin[1] + (cy * SUB + ly - BOX_MARGIN) * sub_size
    x1, y1 = x0 + (1.0 + 2.0 * BOX_MARGIN) * sub_size, y0 + (1.0 + 2.0 * BOX_MARGIN) * sub_size
    occ_cell = cells6[:, 5] >= 5.0
    bound = np.full(rows * cols, -np.inf)
    self_occ = np.zeros(rows * cols, bool)
    for b in (-1, 0, 1):
        for a in (-1, 0, 1):
            touch = ((a == 0) | ((a < 0) & (lx == 0)) | ((a > 0) & (lx == SUB - 1))) & \
                    ((b == 0) | ((b < 0) & (ly == 0)) | ((b > 0) & (ly == SUB - 1)))
            nx, ny = cx + a, cy + b
            ok = touch & (nx >= 0) & (nx < sx) & (ny >= 0) & (ny < sy)
            cell = np.where(ok, ny * sx + nx, 0)
            ok &= occ_cell[cell]
            r = cells6[cell]
            e = exponent_upper_bound((r[:, 0], r[:, 1], -0.5 * r[:, 2], -0.5 * r[:, 3], -0.5 * r[:, 4]), x0, x1, y0, y1)
            bound = np.where(ok, np.maximum(bound, e), bound)
            if a == 0 and b == 0:
                self_occ = ok
    level = np.zeros(rows * cols, np.int64)
    has = bound > -np.inf
    with np.errstate(invalid="ignore"):
        lv = np.where(bound > 0.0, 63, np.where(bound < -62.0, 1, 63 + np.ceil(np.minimum(np.maximum(bound, -63.0), 0.0))))
    level[has] = lv[has].astype(np.int64)
    return level.reshape(rows, cols), self_occ.reshape(rows, cols)


def skip_of(total):
    """(skip_below, skip_level) per lane: negligible_below + skip_state."""
    k = np.frexp(np.where(total > 0.0, total, 1.0))[1] - 1
    from_sum = k * LN2 - 38.0
    below = np.where((total > 0.0) & (from_sum > -746.0), from_sum, -746.0)
    return below, np.clip(np.ceil(below).astype(np.int64) + 63, 1, 63)


def main():
    stride = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    params = synth.matcher_params(CFG)
    m = oracle_lib.ScanMatcherNDT()
    m.initialize(**params)
    m.addScans(synth.map_scans(CFG))
    ndt = m.ndt
    sx, sy, c, origin = ndt.size_x, ndt.size_y, ndt.cell_size, ndt.origin
    cells6 = ndt.cells6()
    guess, pts, _ = synth.query_scan(CFG)
    dlin = oracle_lib.search_offsets(params["search_linear_size"], params["search_linear_resolution"])
    dth = oracle_lib.search_offsets(params["search_angular_size"], params["search_angular_resolution"])
    n_lin, n_th, n_b = len(dlin), len(dth), len(pts)
    # lane_geometry: the whole grid is the window here
    lin_cells = np.abs(dlin).max() / c
    pad = int(2.0 * lin_cells) + 3
    w_cells, h_cells = sx + 2 * pad, sy + 2 * pad
    assert w_cells * SUB <= 256 and h_cells * SUB <= 256
    unit = 65536.0 * SUB
    inv_scaled = unit / c
    level, occupied = map_levels(cells6, sx, sy, c, origin, pad, w_cells, h_cells)
    span_units = math.ceil((dlin[7] - dlin[0]) * inv_scaled) + 2.0
    box = int(math.floor((65535.0 + span_units) / 65536.0))
    assert box <= 3
    d_units = np.rint(dlin * inv_scaled).astype(np.int64)
    rec_h = np.column_stack([cells6[:, 0], cells6[:, 1], -0.5 * cells6[:, 2], -0.5 * cells6[:, 3], -0.5 * cells6[:, 4]])
    can_score_cell = cells6[:, 5] >= 5.0

    names = ("lookup_groups", "live_groups", "live_beams", "exact_evaluations", "exp",
             "groups_or_chunk", "groups_max_chunk", "groups_or_group")
    count = dict.fromkeys(names, 0)
    items = 0
    for t in range(0, n_th, stride):
        th = guess[2] + dth[t]
        ct, st = math.cos(th), math.sin(th)
        ox = pts[:, 0] * ct - pts[:, 1] * st + guess[0]
        oy = pts[:, 0] * st + pts[:, 1] * ct + guess[1]
        kx = np.rint(((ox - origin[0]) / c + pad) * unit).astype(np.int64) + NEAR_UNITS
        ky = np.rint(((oy - origin[1]) / c + pad) * unit).astype(np.int64) + NEAR_UNITS
        for pxi in range(n_lin // 8):
            for pyi in range(n_lin // 8):
                items += 1
                ix = pxi * 8 + np.arange(64) // 8
                iy = pyi * 8 + np.arange(64) % 8
                fx = kx[:, None] + d_units[ix][None, :]            # [beam, lane]
                fy = ky[:, None] + d_units[iy][None, :]
                col, row = fx >> 16, fy >> 16
                lv = level[row, col]
                oc = occupied[row, col]
                near = ((fx & 0xffff) < 2 * NEAR_UNITS) | ((fy & 0xffff) < 2 * NEAR_UNITS)
                # the box of the first lane: OR and maximum of its levels
                c0, r0 = col[:, 0], row[:, 0]
                box_or = np.zeros(n_b, np.int64)
                box_max = np.zeros(n_b, np.int64)
                for r in range(box + 1):
                    for q in range(box + 1):
                        v = level[np.minimum(r0 + r, level.shape[0] - 1), np.minimum(c0 + q, level.shape[1] - 1)]
                        box_or |= v
                        box_max = np.maximum(box_max, v)
                total = np.zeros(64)
                below, lanes_level = skip_of(total)
                for b0 in range(0, n_b, 64):
                    chunk_min = lanes_level.min()
                    for g0 in range(b0, min(b0 + 64, n_b), 8):
                        g = slice(g0, min(g0 + 8, n_b))
                        if not box_or[g].any():
                            continue
                        count["lookup_groups"] += 1
                        count["groups_or_chunk"] += bool((box_or[g] >= chunk_min).any())
                        count["groups_max_chunk"] += bool((box_max[g] >= chunk_min).any())
                        count["groups_or_group"] += bool((box_or[g] >= lanes_level.min()).any())
                        live = lv[g] >= lanes_level[None, :]
                        if not live.any():
                            continue
                        count["live_groups"] += 1
                        added = False
                        for u in np.flatnonzero(live.any(axis=1)):
                            b = g0 + u
                            count["live_beams"] += 1
                            if not ((oc[b] | near[b]) & live[u]).any():
                                continue
                            count["exact_evaluations"] += 1
                            px = ox[b] + dlin[ix]
                            py = oy[b] + dlin[iy]
                            gx = ((px - origin[0]) / c).astype(np.int64)
                            gy = ((py - origin[1]) / c).astype(np.int64)
                            ok = (px >= origin[0]) & (py >= origin[1]) & (gx < sx) & (gy < sy)
                            cell = np.where(ok, gy * sx + gx, 0)
                            ok &= can_score_cell[cell]
                            r = rec_h[cell]
                            q0, q1 = px - r[:, 0], py - r[:, 1]
                            e = (q0 * r[:, 2] + q1 * r[:, 3]) * q0 + (q0 * r[:, 3] + q1 * r[:, 4]) * q1
                            e = np.where(ok, e, -np.inf)
                            if (~(e < below)).any():
                                count["exp"] += 1
                                with np.errstate(under="ignore"):
                                    total = total + np.exp(e)
                                added = True
                        if added:
                            below, lanes_level = skip_of(total)
    per = {k: v / items for k, v in count.items()}
    print("cfg-2, %d items (every %d-th theta step, %d whole patches each), per item:" % (items, stride, (n_lin // 8) ** 2))
    for k in names[:5]:
        print("  %-22s %8.1f" % (k, per[k]))
    base = per["lookup_groups"]
    print("look-up groups per item by pre-test (today %.1f; floor = live groups %.1f):" % (base, per["live_groups"]))
    for k, what in (("groups_or_chunk", "box OR >= L_min, L_min taken at chunk start"),
                    ("groups_max_chunk", "exact box maximum, chunk start"),
                    ("groups_or_group", "L_min re-taken at every group")):
        print("  %-46s %6.1f  %+5.1f %%" % (what, per[k], 100.0 * (per[k] / base - 1.0)))


if __name__ == "__main__":
    main()
