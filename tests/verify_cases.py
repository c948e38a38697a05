"""The cases the match verification's tests share (tests/test_verify_host.py on the CPU, which
validates the choice of inputs on the restatement; tests/test_gpu_verify.py on the GPU): two
designed grids whose cell records are the test vectors -- 7 x 13 cells of size 0.75 (divide
indexing) and 8 x 8 cells of size 0.5 (power-of-two indexing) --, the rays through them, the gate
boundary grid, and the two scenarios on cfg-1's map.  Every coordinate of the designed cases is
dyadic, so with theta = 0 every point is formed exactly.  Computed once, left unchanged."""
import numpy as np

import designed_grids as D
import refine_restatement as R
import verify_restatement as V
from ndt_2d_amd import synth

GATE_INLIER, GATE_PIERCE = 9.0, 1.0
# the directions of the rays from the origin cell, in cells: the eight octants and the four half axes
OCTANTS = [(3, 1), (1, 3), (-1, 3), (-3, 1), (-3, -1), (-1, -3), (1, -3), (3, -1)]
AXES = [(3, 0), (0, 3), (-3, 0), (0, -3)]
SHORT = [(0, 0), (1, 0), (0, -1), (1, 1), (2, 0), (-2, 1), (0, 2)]     # rays of 0, 1 and 2 cells


def iso(mean_x, mean_y, information, n=5.0):
    """A record with isotropic information (tests/designed_grids.py records_for, shape "iso")."""
    rec = D.records_for(np.array([-0.5 * information]), mean_x, mean_y, "iso")[0]
    rec[5] = n
    return rec


class Designed:
    """A designed grid: cells6 records, the restatement's view, and the robot's cell."""

    def __init__(self, size_x, size_y, cell, origin, robot_cell, seed):
        self.size_x, self.size_y, self.cell, self.origin = size_x, size_y, float(cell), origin
        self.robot_cell = robot_cell
        self.cells6 = np.zeros((size_x * size_y, 6))
        rng = np.random.default_rng(seed)
        rx, ry = robot_cell
        for gy in range(size_y):
            for gx in range(size_x):
                ring = max(abs(gx - rx), abs(gy - ry))
                # the robot's own cell scores (it is never tested); ring 1 holds the cells at distance 2
                # from the end of a three-cell ray, ring 2 those at distance 1, ring 3 the ends; further
                # out (the 7 x 13 grid's long columns) every other cell scores
                scores = ring <= 3 or (gx + gy) % 2 == 0
                if (gx, gy) in ((0, 0), (size_x - 1, size_y - 1)):
                    scores = False                      # the corner cells themselves are empty: their neighbours decide
                if not scores:
                    continue
                # means on a 1 / 64 lattice inside the cell, information 4 (sd 0.5) or 64 (sd 0.125)
                fx, fy = rng.integers(8, 57, 2) / 64.0
                info = 4.0 if rng.integers(0, 2) else 64.0
                self.cells6[gy * size_x + gx] = iso(origin[0] + cell * (gx + fx), origin[1] + cell * (gy + fy), info)
        # a degenerate cell: infinite information -- an OUTLIER where a beam ends in it, never piercing
        self.degenerate = (rx + 1, ry - 1)
        dx_, dy_ = self.degenerate
        self.cells6[dy_ * size_x + dx_] = [origin[0] + cell * (dx_ + 0.5), origin[1] + cell * (dy_ + 0.5), np.inf, 0.0, np.inf, 5.0]
        self.grid = R.Grid(self.cells6, size_x, size_y, cell, origin)

    def centre(self, gx, gy, fx=0.5, fy=0.5):
        return (self.origin[0] + self.cell * (gx + fx), self.origin[1] + self.cell * (gy + fy))

    def robot(self, fx=0.5, fy=0.5):
        return self.centre(self.robot_cell[0], self.robot_cell[1], fx, fy)

    def ray_targets(self):
        """World points: the ends of the twelve three-cell rays, of the short rays, of rays down
        the long axis of the grid (where it has one), in the degenerate cell, in both corner cells,
        off each side of the grid, and three that are not finite."""
        rx, ry = self.robot_cell
        out = [self.centre(rx + dx, ry + dy, 0.25, 0.625) for dx, dy in OCTANTS + AXES + SHORT]
        for gy in range(self.size_y):
            if abs(gy - ry) > 3:
                out.append(self.centre(rx + (gy % 3) - 1, gy, 0.75, 0.375))
        out.append(self.centre(*self.degenerate))
        out += [self.centre(0, 0, 0.125, 0.125), self.centre(self.size_x - 1, self.size_y - 1, 0.875, 0.875)]
        tiny = self.cell * 2.0 ** -20
        x0, y0 = self.origin
        x1, y1 = x0 + self.cell * self.size_x, y0 + self.cell * self.size_y
        out += [(x0 - tiny, y0 + self.cell), (x1 + tiny, y0 + self.cell), (x0 + self.cell, y0 - tiny), (x0 + self.cell, y1 + tiny)]
        out += [(np.nan, 0.0), (np.inf, 0.0), (0.0, -np.inf)]
        return np.array(out)

    def beams_to(self, pose, targets):
        """Robot-frame beams whose end points at `pose` are the world points `targets` (theta = 0:
        exactly)."""
        c, s = R.cos_sin(pose[2])
        with np.errstate(invalid="ignore"):
            d = np.asarray(targets, dtype=np.float64) - np.array(pose[:2])
            return np.column_stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]])

    def jobs(self):
        """(poses [K, 3], scans, job_scan): the robot in its cell looking along x; the same scan
        from a turned pose; a robot in column gx = 0 looking up the column; a robot off the grid."""
        pose0 = self.robot() + (0.0,)
        scan0 = self.beams_to(pose0, self.ray_targets())
        pose1 = self.robot(0.25, 0.75) + (0.3,)
        col = self.centre(0, 1, 0.5, 0.5) + (0.0,)
        column = self.beams_to(col, [self.centre(0, gy, 0.5, 0.25) for gy in range(self.size_y)])
        outside = (self.origin[0] - 1.0, self.origin[1] - 1.0, 0.0)
        scan_out = self.beams_to(outside, self.ray_targets()[:12])
        poses = np.array([pose0, pose1, col, outside])
        return poses, [scan0, column, scan_out], [0, 0, 1, 2]


_DESIGNED = {}


def designed(which):
    """"divide": 7 x 13 cells of 0.75; "pow2": 8 x 8 cells of 0.5."""
    if which not in _DESIGNED:
        if which == "divide":
            _DESIGNED[which] = Designed(7, 13, 0.75, (-1.5, -3.0), (3, 6), 41)
        else:
            _DESIGNED[which] = Designed(8, 8, 0.5, (-2.0, -2.0), (4, 4), 43)
    return _DESIGNED[which]


def boundary_grid():
    """Identity information and offsets that put values exactly on the gates.  8 x 8 cells of 1.0
    from (0, 0); the robot at (0.5, 4.5) looks along x.
      cell (6, 4): mean 2.0 to the left of the beam end (6.5, 4.5): m2 = 4.0 exactly.
      cell (2, 4): mean (2.5, 6.5), 2.0 above the segment at t = 0.5 exactly for the beam to (4.5, 4.5):
                   u = (4, 0), w = (2, 2), D = 16, N = 8, t = 0.5, r = (0, 2), r^T I r = 4.0 exactly.
    Returns (grid, pose, beams): beam 0 ends in (6, 4), beam 1 in (4, 4)."""
    cells6 = np.zeros((64, 6))
    cells6[4 * 8 + 6] = iso(4.5, 4.5, 1.0)
    cells6[4 * 8 + 2] = iso(2.5, 6.5, 1.0)
    grid = R.Grid(cells6, 8, 8, 1.0, (0.0, 0.0))
    pose = (0.5, 4.5, 0.0)
    beams = np.array([[6.0, 0.0], [4.0, 0.0]])
    return grid, pose, beams


def tie_grid():
    """Two neighbours of a beam's own cell whose means lie symmetric about the point with the same
    information: equal m2, the lower j wins.  4 x 4 cells of 1.0 from (0, 0); the point (1.5, 1.5) in
    cell (1, 1); neighbours j = 3 (cell (0, 1)) and j = 5 (cell (2, 1)), means 1.0 either side; the own
    cell and the others are empty.  Returns (grid, pose, beams)."""
    cells6 = np.zeros((16, 6))
    cells6[1 * 4 + 0] = iso(0.5, 1.5, 2.0)
    cells6[1 * 4 + 2] = iso(2.5, 1.5, 2.0)
    grid = R.Grid(cells6, 4, 4, 1.0, (0.0, 0.0))
    return grid, (1.5, 0.5, 0.0), np.array([[0.0, 1.0]])


def wrap_grid():
    """The clip on (gx, gy): 4 x 4 cells of 1.0 from (0, 0), the only scoring cell is (3, 0) -- the
    flat index of cell (0, 1) minus one.  A beam that ends in (0, 1) has no counting neighbour
    (UNSEEN); one that ends in (2, 1) has (neighbour j = 2).  Returns (grid, pose, beams)."""
    cells6 = np.zeros((16, 6))
    cells6[3] = iso(3.5, 0.5, 1.0)
    grid = R.Grid(cells6, 4, 4, 1.0, (0.0, 0.0))
    return grid, (1.5, 2.5, 0.0), np.array([[-1.0, -1.0], [1.0, -1.0]])


# ---- the scenarios on cfg-1's map ----

_SCENARIO = {}


def oracle_grid_of(scans, params):
    import oracle_lib as O
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans(scans)
    return ref, R.Grid.of_oracle(ref)


def scenario():
    """cfg-1's map (41 x 41) and its 720-beam query; jobs: the true pose, + 1 m in x, + 0.3 rad."""
    if "poses" not in _SCENARIO:
        scans = synth.map_scans(1)
        params = synth.matcher_params(1)
        _, pts, true_pose = synth.query_scan(1)
        ref, grid = oracle_grid_of(scans, params)
        jobs = np.array([true_pose, true_pose + (1.0, 0.0, 0.0), true_pose + (0.0, 0.0, 0.3)])
        _SCENARIO["poses"] = dict(scans=scans, params=params, query=pts, true_pose=true_pose, jobs=jobs, ref=ref, grid=grid)
    return _SCENARIO["poses"]


def pillar_scenario():
    """The map of cfg-1's world (pillars at (+-2, +-2), half width 0.25); the query from cfg-1's
    true pose in the same room WITHOUT the pillars: the beams the pillars used to stop reach the wall."""
    if "pillars" not in _SCENARIO:
        s = scenario()
        half, pitch, _ = synth.CONFIGS[1]["world"]
        empty_room = synth.world_of((half, pitch, 0.0))
        query = synth.scan(empty_room, s["true_pose"], synth.CONFIGS[1]["query"]["seed"])
        _SCENARIO["pillars"] = dict(s, query=query, jobs=np.array([s["true_pose"]]))
    return _SCENARIO["pillars"]


def near_a_pillar(grid, cell, margin_cells=1):
    """Does the flat cell lie within margin_cells cells of one of cfg-1's pillars?"""
    gy, gx = divmod(int(cell), grid.size_x)
    x0, y0 = grid.origin[0] + grid.cell_size * gx, grid.origin[1] + grid.cell_size * gy
    x1, y1 = x0 + grid.cell_size, y0 + grid.cell_size
    m = margin_cells * grid.cell_size
    for px in (-2.0, 2.0):
        for py in (-2.0, 2.0):
            if x1 >= px - 0.25 - m and x0 <= px + 0.25 + m and y1 >= py - 0.25 - m and y0 <= py + 0.25 + m:
                return True
    return False
