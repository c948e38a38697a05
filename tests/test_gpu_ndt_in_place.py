"""The NDT in place of a matcher (csrc/host/ndt2d_matcher_state.h NdtInPlace) through every way it
changes, in ONE matcher: host build, reset, device build, scans stored beside it, a refused and a
good addScansById, a host build again, matchCandidates.  After each step: has_ndt, last_build, and
scoreScan of the query scan == that of a fresh matcher brought to the same state directly (0.0 where no
NDT is in place) -- whatever an earlier state left behind (a host copy, a copy fetched back from
the device, spare storage) must not show."""
import numpy as np
import pytest

from ndt_2d_amd import Ndt2dError, ScanMatcherNDT, _capi, synth

pytestmark = pytest.mark.gpu

CFG = 1   # 41 x 41 cells, 100 beams: the smallest map of the suite


def _fresh(mode, scans=None, stored=None):
    """A new matcher with an NDT built one way: addScans(scans) under `mode`, or addScansById of `stored`."""
    f = ScanMatcherNDT(0)
    f.initialize("fresh", **synth.matcher_params(CFG))
    f.set_build_mode(mode)
    if stored is not None:
        ids = [f.storeScan(pts) for _, pts in stored]
        f.addScansById([pose for pose, _ in stored], ids)
    elif scans is not None:
        f.addScans(scans)
    return f


def test_the_ndt_in_place_through_every_transition():
    scans = synth.map_scans(CFG)
    guess, pts, _ = synth.query_scan(CFG)
    window = scans[:3]

    def expect(m, build, fresh):
        """has_ndt, last_build and the score, which is the fresh matcher's."""
        try:
            want = fresh.scoreScan(guess, pts) if fresh is not None else 0.0
            assert (fresh.last_build() if fresh is not None else "") == build
        finally:
            if fresh is not None:
                fresh.close()
        got = (bool(m.has_ndt()), m.last_build(), m.scoreScan(guess, pts))
        assert got == (build != "", build, want), (got, want)
        assert build == "" or want < 0.0
        return got

    m = ScanMatcherNDT(0)
    try:
        m.initialize("walk", **synth.matcher_params(CFG))
        # 1. host build
        m.set_build_mode("host")
        m.addScans(scans)
        expect(m, "build/host", _fresh("host", scans))
        # 2. reset
        m.reset()
        expect(m, "", None)
        # 3. device build: no host copy; the single pose is scored from the grid fetched back
        m.set_build_mode("device")
        m.addScans(scans)
        expect(m, "build/device", _fresh("device", scans))
        # 4. scans stored beside it: the NDT in place is not touched
        ids = [m.storeScan(p) for _, p in window]
        assert ids == [0, 1, 2]
        before = expect(m, "build/device", _fresh("device", scans))
        # 5. an unknown id is refused by the first store: everything stays
        with pytest.raises(Ndt2dError) as ei:
            m.addScansById([pose for pose, _ in window], [0, 1, 3])
        assert ei.value.code == _capi.ERR_INVALID and "unknown scan id" in str(ei.value)
        assert (bool(m.has_ndt()), m.last_build(), m.scoreScan(guess, pts)) == before
        # 6. the stored scans built on the device (the fused build): scored there, no fetched copy
        m.addScansById([pose for pose, _ in window], ids)
        expect(m, "build/fused-small-map", _fresh("device", stored=window))
        # 7. a host build again: the single pose is scored from the rebuilt host copy
        m.set_build_mode("host")
        m.addScans(scans)
        expect(m, "build/host", _fresh("host", scans))
        # 8. matchCandidates ends with no NDT in place
        cands = [[(0, window[0][0]), (1, window[1][0])], [(2, window[2][0])]]
        got = m.matchCandidates(guess, pts, cands)
        assert len(got) == 2 and all(np.isfinite(g["score"]) for g in got)
        expect(m, "", None)
        assert m.has_ndt() == 0 and m.last_build() == ""
    finally:
        m.close()
