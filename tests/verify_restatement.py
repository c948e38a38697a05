"""The match verification (include/ndt2d_hip.h, "Match verification") restated on the CPU: Python
floats (IEEE doubles, no fused multiply-add) and integers over the oracle's cells6 records, libm's
sincos, every operation in the order the contract gives.  Written from the contract, not from the
kernel.  Test infrastructure only: the yardstick of tests/test_verify_host.py (which pins it to the
oracle's likelihood_point and to the oracle's occupancy renderer) and tests/test_gpu_verify.py.
It reuses refine_restatement.Grid (the records and NDT::getIndex).
"""
import math

import numpy as np

import refine_restatement as R

OFF, UNSEEN, OUTLIER, INLIER = 0, 1, 2, 3
PIERCED = 4
NO_CELL = 0xFFFFFFFF
RECORD_U32 = 8


def line_cells(ox, oy, gx, gy):
    """The cells the integer line from (ox, oy) to (gx, gy) visits, in order: the all-octant error
    form of the contract.  Python integers."""
    dx, dy = abs(gx - ox), -abs(gy - oy)
    sx = 1 if ox < gx else -1
    sy = 1 if oy < gy else -1
    err = dx + dy
    x, y = ox, oy
    cells = [(x, y)]
    while len(cells) < dx - dy + 1:
        if x == gx and y == gy:
            break
        if 2 * err >= dy:
            if x == gx:
                break
            err += dy
            x += sx
        if 2 * err <= dx:
            if y == gy:
                break
            err += dx
            y += sy
        cells.append((x, y))
    return cells


def testable_cells(cells, origin, end):
    """Of a line's visited cells, those that are tested if they can score: not the origin cell,
    Chebyshev distance to the end cell > 1."""
    return [(x, y) for x, y in cells if (x, y) != tuple(origin) and max(abs(end[0] - x), abs(end[1] - y)) > 1]


def cell_m2(rec, qx, qy):
    """m2 = d^T I d as -2 x Cell::score's exponent on h = -0.5 I."""
    h00, h01, h11 = -0.5 * rec[2], -0.5 * rec[3], -0.5 * rec[4]
    with np.errstate(all="ignore"):
        q0 = np.float64(qx) - rec[0]
        q1 = np.float64(qy) - rec[1]
        r0 = q0 * h00 + q1 * h01
        r1 = q0 * h01 + q1 * h11
        return float(-2.0 * (r0 * q0 + r1 * q1))


def approach(ux, uy, wx, wy, i00, i01, i11):
    """r^T I r at the closest approach of the segment to the mean, the contract's operation order."""
    with np.errstate(all="ignore"):
        ux, uy, wx, wy = np.float64(ux), np.float64(uy), np.float64(wx), np.float64(wy)
        i00, i01, i11 = np.float64(i00), np.float64(i01), np.float64(i11)
        iu0 = i00 * ux + i01 * uy
        iu1 = i01 * ux + i11 * uy
        D = ux * iu0 + uy * iu1
        N = wx * iu0 + wy * iu1
        t = N / D
        if not D > 0.0:
            t = np.float64(0.0)
        if not t >= 0.0:
            t = np.float64(0.0)
        elif t > 1.0:
            t = np.float64(1.0)
        rx = wx - t * ux
        ry = wy - t * uy
        ir0 = i00 * rx + i01 * ry
        ir1 = i01 * rx + i11 * ry
        return float(rx * ir0 + ry * ir1)


def neighbours(grid, own, cells):
    """The cells of a point's neighbourhood that lie on the grid, in ascending j: clipped on
    (gx, gy), never on the flat index."""
    if cells == 1:
        return [own]
    gy, gx = divmod(own, grid.size_x)
    out = []
    for j in range(9):
        nx, ny = gx + j % 3 - 1, gy + j // 3 - 1
        if 0 <= nx < grid.size_x and 0 <= ny < grid.size_y:
            out.append(ny * grid.size_x + nx)
    return out


def verify(grid, beams, pose, neighbourhood=1, gate_inlier=9.0, gate_pierce=1.0, rays=True, cs=None):
    """One job.  Returns dict(record[8], classes[n] (the two low bits), pierced_mask[n], m2[n],
    cells[n, 2], tested = per beam the list of (cell, r^T I r) of the cells tested up to and
    including the first piercing one, visited = per beam the line's cells as flat indices (empty
    where no ray is walked)).  cs: (cos, sin) of the heading, libm's sincos pair if not given."""
    b = np.ascontiguousarray(beams, dtype=np.float64).reshape(-1, 2)
    x, y = float(pose[0]), float(pose[1])
    c, s = R.cos_sin(pose[2]) if cs is None else cs
    n = len(b)
    with np.errstate(all="ignore"):
        qx = c * b[:, 0] - s * b[:, 1] + x
        qy = s * b[:, 0] + c * b[:, 1] + y
        own = grid.index(qx, qy)
    origin = int(grid.index(np.array([x]), np.array([y]))[0])
    classes = np.zeros(n, dtype=np.uint8)
    pierced = np.zeros(n, dtype=bool)
    m2 = np.full(n, np.inf)
    cells = np.full((n, 2), NO_CELL, dtype=np.uint32)
    tested, visited = [], []
    walked = 0
    for i in range(n):
        tested.append([])
        visited.append([])
        if own[i] < 0:
            classes[i] = OFF
            continue
        best, won = None, None
        for cell in neighbours(grid, int(own[i]), neighbourhood):
            rec = grid.cells[cell]
            if not rec[5] >= 5:
                continue
            v = cell_m2(rec, qx[i], qy[i])
            # numpy's argmin: below the held one, or NaN while the held one is not
            if won is None or (best == best and not v >= best):
                best, won = v, cell
        if won is None:
            classes[i] = UNSEEN
        else:
            classes[i] = INLIER if best <= gate_inlier else OUTLIER
            m2[i] = best
            cells[i, 0] = won
        if not rays or origin < 0:
            continue
        walked += 1
        oy, ox = divmod(origin, grid.size_x)
        gy, gx = divmod(int(own[i]), grid.size_x)
        line = line_cells(ox, oy, gx, gy)
        visited[i] = [cy * grid.size_x + cx for cx, cy in line]
        ux, uy = float(qx[i] - np.float64(x)), float(qy[i] - np.float64(y))
        for cx, cy in testable_cells(line, (ox, oy), (gx, gy)):
            cell = cy * grid.size_x + cx
            rec = grid.cells[cell]
            if not rec[5] >= 5:
                continue
            rIr = approach(ux, uy, rec[0] - np.float64(x), rec[1] - np.float64(y), rec[2], rec[3], rec[4])
            tested[i].append((cell, rIr))
            if rIr <= gate_pierce:
                pierced[i] = True
                cells[i, 1] = cell
                break
    record = np.array([n, int(np.sum(classes == OFF)), int(np.sum(classes == UNSEEN)), int(np.sum(classes == OUTLIER)),
                       int(np.sum(classes == INLIER)), int(np.sum(pierced)), walked, 0], dtype=np.uint32)
    return dict(record=record, classes=classes, pierced_mask=pierced, m2=m2, cells=cells, tested=tested, visited=visited)


def near_gate(result, gate_inlier, gate_pierce, rel=1e-8):
    """The beams whose m2, or one of whose tested cells' r^T I r, lies within `rel` (relative) of
    its gate: there a last-bit difference could change a class or a pierce flag."""
    out = []
    for i, v in enumerate(result["m2"]):
        close = math.isfinite(v) and abs(v - gate_inlier) <= rel * max(abs(gate_inlier), abs(v))
        for _, r in result["tested"][i]:
            close = close or (math.isfinite(r) and abs(r - gate_pierce) <= rel * max(abs(gate_pierce), abs(r)))
        if close:
            out.append(i)
    return out
