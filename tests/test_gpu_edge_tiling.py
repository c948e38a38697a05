"""Strip tiles at the lattice edge of the large lane search (lane_tiling, csrc/ndt2d_lane_fn.h).

Where n_lin leaves 1..4 steps behind its last whole group of eight, the unsplit dynamic-item
forms cut the last row and column of 8 x 8 patches into strips of 4 x 16, 2 x 32 or 1 x 64.  A
candidate's score must not depend on the tile that holds it, every candidate must be held by
exactly one tile, and neither may depend on how theta is sharded or cut into slabs.

The 41 x 41 cfg-1 map, 720 beams (the dynamic-item forms run from 256), 3 theta steps, the lane
search forced with the variant knob.  Lattices this small would have their beams cut into parts
(the beam-part kernels keep 8 x 8 patches), so NDT2D_LANE_PARTS=1 -- the library's own A/B knob --
keeps the search unsplit; every test asserts that it ran that way.

The lattice steps are powers of two, so that `for (v = -size; v < size; v += res)` takes exactly
n_lin steps.  Two lattices fall back to 8 x 8 patches: one so coarse (0.125 m steps on 0.25 m
cells: 16 steps span 7.5 sub-cells) that even a patch outgrows its pre-test, and one (27/256 m
steps, n_lin = 18: the 2 x 32 strip spans 7.2 sub-cells, a patch 2.95) where only the strip does.
"""
import math

import numpy as np
import pytest

import oracle_lib as O
from ndt_2d_amd import ScanMatcherNDT, synth
from ndt_2d_amd import dist as shard

pytestmark = pytest.mark.gpu

RES = 2.0 ** -6          # 16 steps = 0.23 m: within one 0.25 m cell of the corner
ANG_RES = 2.0 ** -8
N_TH = 3
CASES = {("n%d" % n): (n, RES) for n in (1, 4, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 20)}
CASES["coarse20"] = (20, 0.125)
CASES["coarse18"] = (18, 27.0 / 256.0)

_cache = {}


@pytest.fixture(autouse=True)
def _unsplit(monkeypatch):
    monkeypatch.setenv("NDT2D_LANE_PARTS", "1")


def _offsets(size, res):
    out, v = [], -size
    while v < size:
        out.append(v)
        v += res
    return np.array(out)


def _nan_launch(gpu, launch, n):
    """Scores of a launch into a buffer pre-filled with NaN, and the launch's record."""
    import torch
    d = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    launch(d.data_ptr())
    gpu.synchronize()
    rec = gpu.match_fetch()
    assert "lane-per-candidate" in gpu.last_variant() and "beam-parts" not in gpu.last_variant()
    return d.cpu().numpy(), rec


def _case(name):
    """One matcher and one oracle result per lattice, shared by the tests below."""
    if name in _cache:
        return _cache[name]
    n_lin, res = CASES[name]
    params = synth.matcher_params(1, search_linear_size=n_lin * res / 2, search_linear_resolution=res,
                                  search_angular_size=N_TH * ANG_RES / 2, search_angular_resolution=ANG_RES)
    scans = synth.map_scans(1)
    guess, pts, _ = synth.query_scan(1)
    gpu = ScanMatcherNDT(0)
    gpu.initialize("edge", **params)
    gpu.addScans(scans)
    gpu.set_timing(True)   # (last_launch_ms: the kernels of a launch are counted)
    ref = O.ScanMatcherNDT()
    ref.initialize(**params)
    ref.addScans(scans)
    exp = ref.matchScan(guess, pts, want_scores=True)
    assert gpu.prepare_search(guess, pts) == (N_TH, n_lin, 720)
    c = dict(gpu=gpu, n_lin=n_lin, per=n_lin * n_lin, oracle=exp["scores"],
             dlin=_offsets(n_lin * res / 2, res), dth=_offsets(N_TH * ANG_RES / 2, ANG_RES))
    assert len(c["dlin"]) == n_lin and len(c["dth"]) == N_TH
    gpu.set_variant("lane")
    c["scores"], c["record"] = _nan_launch(gpu, lambda p: gpu.match_launch(0, N_TH, scores_ptr=p), N_TH * c["per"])
    gpu.set_variant("lane-noskip")
    c["noskip"], c["noskip_record"] = _nan_launch(gpu, lambda p: gpu.match_launch(0, N_TH, scores_ptr=p),
                                                  N_TH * c["per"])
    gpu.set_variant("lane")
    _cache[name] = c
    return c


@pytest.mark.parametrize("name", list(CASES))
def test_every_candidate_is_scored_once_with_the_same_bits(name):
    c = _case(name)
    assert not np.isnan(c["scores"]).any() and not np.isnan(c["noskip"]).any()
    assert np.array_equal(c["scores"], c["noskip"])
    err = float(np.max(np.abs(c["scores"] - c["oracle"])))
    print("%s: max |score - oracle| = %.3e" % (name, err))
    assert err < 1e-9
    assert (c["scores"] < 0).any()


@pytest.mark.parametrize("name", list(CASES))
def test_record_is_the_first_wins_argmin_and_the_sums_of_the_scores(name):
    c = _case(name)
    s, n_lin = c["scores"], c["n_lin"]
    for rec in (c["record"], c["noskip_record"]):
        assert rec[0] == s.min() and math.floor(rec[1]) == int(np.argmin(s))   # (argmin: the first of equals)
        dt = np.repeat(c["dth"], n_lin * n_lin)
        dx = np.tile(np.repeat(c["dlin"], n_lin), N_TH)
        dy = np.tile(c["dlin"], N_TH * n_lin)
        terms = [(dx * dx) * s, (dx * dy) * s, (dx * dt) * s, (dy * dy) * s, (dy * dt) * s, (dt * dt) * s,
                 dx * s, dy * s, dt * s, s]
        for k, term in enumerate(terms):
            want = math.fsum(term)
            print("%s acc[%d]: got %.17g want %.17g rel %.2e" % (name, k, rec[2 + k], want,
                                                                 abs(rec[2 + k] - want) / abs(want)))
            assert abs(rec[2 + k] - want) <= 1e-12 * abs(want), (k, rec[2 + k], want)


@pytest.mark.parametrize("name", list(CASES))
def test_theta_shares_and_slabs_give_the_same_scores_and_winner(name, monkeypatch):
    c = _case(name)
    gpu, per = c["gpu"], c["per"]
    whole = shard.combine_match_records([c["record"]])
    for world in (2, 3):
        records = []
        for rank in range(world):
            first, stride, count = shard.shard_strided(N_TH, rank, world)
            got, rec = _nan_launch(
                gpu, lambda p: gpu.match_launch_strided(first, stride, count, scores_ptr=p), count * per)
            mine = np.concatenate([c["scores"][t * per:(t + 1) * per] for t in range(first, N_TH, stride)])
            assert np.array_equal(got, mine)
            records.append(rec)
        best_score, best_index, acc = shard.combine_match_records(records)
        assert (best_score, best_index) == whole[:2]
        assert np.allclose(acc, whole[2], rtol=1e-11, atol=0)
    # one theta step per slab
    monkeypatch.setenv("NDT2D_LANE_SLAB_ITEMS", "1")
    got, rec = _nan_launch(gpu, lambda p: gpu.match_launch(0, N_TH, scores_ptr=p), N_TH * per)
    assert gpu.last_launch_ms()[1] == 3 * N_TH + 1
    assert np.array_equal(got, c["scores"])
    assert (rec[0], rec[1]) == (c["record"][0], c["record"][1])
    assert np.allclose(rec[2:], c["record"][2:], rtol=1e-11, atol=0)
