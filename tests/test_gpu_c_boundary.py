"""Nothing unwinds through the C boundary (csrc/ndt2d_guard.h; SURVEY.md 8b "Errors": the
plugin's callers -- rclcpp's executor threads -- expect no exception): inputs that would size a
container beyond memory come back as a status, the matcher stays usable, and the next valid
call gives the oracle's answer."""
import numpy as np
import pytest

import oracle_lib as O
from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, synth




@pytest.fixture()
def matcher():
    m = ScanMatcherNDT(0)
    yield m
    m.close()


def _expect(code, fn):
    with pytest.raises(Ndt2dError) as e:
        fn()
    assert e.value.code == code, e.value
    return e.value


@pytest.mark.gpu
@pytest.mark.parametrize("bad_pose", [(1e15, 0.0, 0.0), (0.0, -1e15, 0.0), (float("nan"), 0.0, 0.0),
                                      (0.0, float("inf"), 0.0), (0.0, 0.0, float("nan"))])
def test_add_scans_with_an_absurd_pose_is_a_status_and_the_matcher_lives(matcher, bad_pose):
    p = synth.matcher_params(1)
    matcher.initialize("guard", **p)
    scans = synth.map_scans(1)
    bad = list(scans) + [(bad_pose, scans[0][1])]
    _expect(_capi.ERR_INVALID, lambda: matcher.addScans(bad))
    # no NDT after the failed call: the reference's "no map yet" answers (src/scan_matcher_ndt.cpp:80,159)
    guess, pts, _ = synth.query_scan(1)
    assert matcher.scoreScan(guess, pts) == 0.0
    # ... and a valid map afterwards searches to the oracle's result
    matcher.addScans(scans)
    got = matcher.matchScan(guess, pts)
    ref = O.ScanMatcherNDT()
    ref.initialize(**p)
    ref.addScans(scans)
    exp = ref.matchScan(guess, pts)
    assert got["best_index"] == exp["best_index"] and abs(got["score"] - exp["score"]) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("range_max", [float("inf"), float("nan"), -float("inf")])
def test_initialize_refuses_a_non_finite_range_max(matcher, range_max):
    p = dict(synth.matcher_params(1), range_max=range_max)
    _expect(_capi.ERR_INVALID, lambda: matcher.initialize("guard", **p))


@pytest.mark.gpu
def test_a_range_max_that_needs_2_to_the_31_cells_is_refused_before_allocating(matcher):
    p = dict(synth.matcher_params(1), range_max=1.0e7)       # 8e7 x 8e7 cells
    matcher.initialize("guard", **p)
    _expect(_capi.ERR_INVALID, lambda: matcher.addScans(synth.map_scans(1)))
    for mode in ("device", "host"):
        matcher.set_build_mode(mode)
        _expect(_capi.ERR_INVALID, lambda: matcher.addScans(synth.map_scans(1)))


@pytest.mark.gpu
@pytest.mark.parametrize("override", [
    dict(search_linear_size=5.0, search_linear_resolution=1e-5, search_angular_size=0.5,
         search_angular_resolution=0.005),                    # 10^6 x 10^6 x 200 = 2 x 10^14 candidates
    dict(search_linear_size=float("inf")), dict(search_angular_resolution=float("nan")),
    dict(search_angular_size=1e6, search_angular_resolution=1e-6),
    dict(search_linear_size=1.0, search_linear_resolution=1e-300)])
def test_a_lattice_beyond_any_search_is_refused_at_initialize(matcher, override):
    """2^40 candidates and more: the offsets alone would fill the host's memory (the reference's
    loops, src/scan_matcher_ndt.cpp:103,117,119, would simply never return)."""
    p = dict(synth.matcher_params(1), **override)
    _expect(_capi.ERR_INVALID, lambda: matcher.initialize("guard", **p))
    # the matcher keeps the parameters it had and still works
    good = synth.matcher_params(1)
    matcher.initialize("guard", **good)
    matcher.addScans(synth.map_scans(1))
    guess, pts, _ = synth.query_scan(1)
    assert matcher.matchScan(guess, pts)["best_index"] is not None


def test_every_multi_line_entry_point_is_guarded():
    """The two macros bracket every extern "C" body of the host and device layers (a new entry
    point without them fails here, not in production)."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ndt_2d_amd", "csrc")
    missing = []
    host = sorted(os.path.join("host", f) for f in os.listdir(os.path.join(root, "host")) if f.endswith(".cpp"))
    assert len(host) >= 5, host
    device = sorted(os.path.join("device", f) for f in os.listdir(os.path.join(root, "device")) if f.endswith(".hip"))
    assert len(device) >= 5, device
    for name in ["ndt2d_host.cpp"] + host + device:
        lines = open(os.path.join(root, name)).read().split("\n")
        for i, ln in enumerate(lines):
            m = re.match(r'^(?:extern "C" )?int (ndt2d_\w+)\(', ln)
            if not m:
                continue
            j = i
            while lines[j] != "{" and "{" not in lines[j]:
                j += 1
            if lines[j] != "{":
                continue                                  # a one-line accessor
            k = j + 1
            while lines[k] != "}":
                k += 1
            body = "\n".join(lines[j:k])
            if "NDT2D_C_TRY" not in body and "catch (...)" not in body:
                missing.append(m.group(1))
    assert not missing, missing


@pytest.mark.gpu
def test_destroying_one_context_leaves_the_other_ones_buffers_alone():
    """A context's buffers free themselves with it (csrc/device/ndt2d_context.h): two contexts with the
    same 8 x 8 grid, 16 beams and 3 x 3 x 3 search give the same match, and the second gives it again
    after the first is destroyed -- a destructor that freed what it does not own, or twice, would show here."""
    import ctypes as C
    L = _capi.lib()
    cells = np.zeros((64, 6))
    for j in range(8):
        for i in range(8):
            cells[j * 8 + i] = [0.25 * i + 0.125, 0.25 * j + 0.125, 16.0, 0.0, 16.0, 10.0 if (i + j) % 3 else 0.0]
    ang = np.linspace(0.0, 2.0 * np.pi, 16, endpoint=False)
    beams = np.ascontiguousarray(np.stack([0.6 * np.cos(ang), 0.6 * np.sin(ang)], axis=1))
    dth = np.array([-0.1, 0.0, 0.1])
    ct, st, dlin = np.cos(dth), np.sin(dth), np.array([-0.25, 0.0, 0.25])

    def context():
        h = C.c_void_p()
        assert L.ndt2d_create(C.byref(h), 0) == _capi.OK
        assert L.ndt2d_set_grid(h, _capi.dptr(cells), 8, 8, 0.25, 0.0, 0.0) == _capi.OK
        assert L.ndt2d_set_beams(h, _capi.dptr(beams), 16) == _capi.OK
        assert L.ndt2d_set_search(h, 1.0, 1.0, _capi.dptr(dth), _capi.dptr(ct), _capi.dptr(st), 3,
                                  _capi.dptr(dlin), 3) == _capi.OK
        return h

    def match(h):
        scores, res = np.full(27, 123.0), _capi.MatchResult()
        assert L.ndt2d_match(h, 0, 3, _capi.dptr(scores), C.byref(res)) == _capi.OK, L.ndt2d_last_error(h)
        return scores.tobytes(), bytes(res)

    first, second = context(), context()
    one, two = match(first), match(second)
    assert L.ndt2d_destroy(first) == _capi.OK
    again = match(second)
    assert L.ndt2d_destroy(second) == _capi.OK
    assert one == two == again
    scores = np.frombuffer(one[0])
    assert np.isfinite(scores).all() and (scores != 123.0).all() and scores.min() < scores.max()   # (a search ran)
