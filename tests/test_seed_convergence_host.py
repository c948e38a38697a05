"""The convergence case of global localisation (tests/seed_convergence_case.py) holds on the CPU:
the restated loop -- numpy seeding, the oracle's motion model, scorePoints and updateStatistics, the
host KLD loop -- ends within half an NDT cell of the truth, which is what entitles
tests/test_gpu_seed.py to ask the device filter for one cell.  No GPU."""
import seed_convergence_case as K


def test_the_restated_loop_ends_within_half_a_cell():
    """Recorded here: position error 0.0264 m (half a cell: 0.125 m), heading error 0.0076 rad
    (search_angular_size: 0.2), 1,866 particles kept before the last step."""
    mean, truth, kept = K.restated_loop()
    err_xy, err_th = K.errors(mean, truth)
    print("restated loop: position error %.4f m, heading error %.4f rad, %d particles" % (err_xy, err_th, kept))
    params = K.matcher_params()
    assert err_xy <= 0.5 * params["ndt_resolution"]
    assert err_th < params["search_angular_size"]
    assert K.MIN_PARTICLES <= kept < K.N_PARTICLES           # the set shrank on the way
