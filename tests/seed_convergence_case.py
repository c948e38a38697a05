"""The global-localisation convergence case shared by tests/test_seed_convergence_host.py (the CPU
restatement of the loop) and tests/test_gpu_seed.py (the filter on the device).  Test
infrastructure only.

The world is the generator's smallest (cfg-1: an 8 m room, four pillars), which is symmetric under
quarter turns; the MAP is not: it is built from three scans on an L in one corner, (-3, -3),
(-3, -1) and (-1, -3), with range_max 2.5 m, so the NDT and the free space cover that corner only
and the three turned images of the truth lie in unknown space, where nothing is seeded.  The truth
starts at (-3.4, -3.1, 0.1) and makes ten odometry steps of (0.15 m, 0, 0.03 rad).
"""
import numpy as np

import noise_restatement as N
import oracle_lib as O
import seed_restatement as S
from ndt_2d_amd import synth
from ndt_2d_amd.particle_filter import kld_resample_native

CFG = 1
LATTICE = ((-3.0, -3.0), (-3.0, -1.0), (-1.0, -3.0))
RANGE_MAX = 2.5
MAP_RESOLUTION, OCC_THRESH = 0.05, 0.25
TRUTH_START = (-3.4, -3.1, 0.1)
MOTION = (0.15, 0.0, 0.03)
STEPS = 10
ALPHAS = (0.05, 0.05, 0.05, 0.05, 0.05)
SEED = 2
N_PARTICLES, MIN_PARTICLES = 20000, 500
KLD_ERR, KLD_Z = 0.01, 2.3


def matcher_params():
    p = synth.matcher_params(CFG)
    p["range_max"] = RANGE_MAX
    return p


def map_scans():
    """[(pose, points)] of the three mapping scans, as addScans takes them."""
    w = synth.world_of(CFG)
    return [((x, y, 0.0), synth.scan(w, (x, y, 0.0), 1000003 + k)) for k, (x, y) in enumerate(LATTICE)]


def occupancy_scans(scans):
    """The same scans with the points the mapper drops (beyond range_max) removed."""
    return [(p, pts[np.hypot(pts[:, 0], pts[:, 1]) <= RANGE_MAX]) for p, pts in scans]


def trajectory():
    """[(truth pose after step t, its scan)]: the odometry model without noise."""
    w = synth.world_of(CFG)
    truth = np.array(TRUTH_START, dtype=np.float64)
    out = []
    for t in range(STEPS):
        truth = O.motion_sample(*MOTION, np.array(ALPHAS), truth.reshape(1, 3), np.zeros((1, 3), np.float32))[0][0]
        assert not synth.pose_blocked(w, truth[0], truth[1])
        out.append((truth.copy(), synth.scan(w, truth, 777 + t)))
    return out


def errors(mean, truth):
    return (float(np.hypot(mean[0] - truth[0], mean[1] - truth[1])),
            float(abs((mean[2] - truth[2] + np.pi) % (2.0 * np.pi) - np.pi)))


def restated_loop():
    """The filter's loop on the CPU: numpy seeding (seed_restatement), the oracle's motion model on
    the restated noise stream, the oracle's scorePoints and updateStatistics, the host KLD loop on
    the uniforms the filter's own generator gives.  Returns (mean, truth, particles kept)."""
    scans = map_scans()
    ref = O.ScanMatcherNDT()
    ref.initialize(**matcher_params())
    ref.addScans(scans)
    msg = O.OccupancyGrid(MAP_RESOLUTION, OCC_THRESH).getMsg(occupancy_scans(scans))
    table = S.free_table(msg["data"])
    host_rng = np.random.Generator(np.random.Philox(key=SEED))
    particles = S.sample(SEED, 1, 0, N_PARTICLES, table, msg["width"], msg["origin_x"], msg["origin_y"], msg["resolution"])
    step = 2                                                      # init_global took steps 1 and 2
    steps = trajectory()
    for t, (truth, points) in enumerate(steps):
        step += 1
        z, _ = N.normals_reference(SEED, step, 0, len(particles))
        particles = O.motion_sample(*MOTION, np.array(ALPHAS), particles, z.astype(np.float32))[0]
        weights, mean, _ = O.pf_update_statistics(particles, O.pf_measure(ref, particles, points))
        if t + 1 < len(steps):
            keep = kld_resample_native(particles, weights, MIN_PARTICLES, N_PARTICLES, KLD_ERR, KLD_Z,
                                       host_rng.random(N_PARTICLES))
            particles = particles[keep]
    return mean, steps[-1][0], len(particles)
