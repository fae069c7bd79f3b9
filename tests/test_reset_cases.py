"""CPU: the premise of the receive loops' reset tests (tests/test_reset_gpu.py), held on the oracle.  After the stream X of
tests/reset_cases.py every channel holds a sync, stands inside a frame, and has its slicer words away from their reset values - so an
object that runs X and is then reset has something to forget.  The same stream Y holds syncs (and, with the handlers on, decisions)
for the object to find afterwards."""
import numpy as np
import pytest

import orc
import reset_cases as rc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("handlers", [False, True])
def test_p25_streams(built, handlers):
    x, y, locks = rc.p25_case()
    if handlers:
        x = rc.p25_handler_x()
    assert x.shape == (rc.P25_B, rc.P25_N) and y.shape == (rc.P25_B, 2 * rc.P25_N)
    for c in range(rc.P25_B):
        o = rc.p25_oracle(handlers, locks[c])
        fresh = o.thresholds()
        _, _, fl = o.run(x[c])
        assert (fl & 2).any() and fl[-1] & 1, c                                        # a sync was accepted, X ends inside a frame
        if handlers:                                                                   # ... whose NID the handler decoded
            assert any(e[1] == orc.HEV_P25_NID and e[2] > 0 for e in o.events.rows()), c
        assert not np.array_equal(_bits(o.thresholds()), _bits(fresh)), c
        stale, new = o.run(y[c, :rc.P25_N]), rc.p25_oracle(handlers, locks[c]).run(y[c, :rc.P25_N])
        assert len(stale[0]) != len(new[0]) or not np.array_equal(stale[1], new[1]) or not np.array_equal(stale[2], new[2]), c
        o = rc.p25_oracle(handlers, locks[c])
        _, _, fl = o.run(y[c])
        assert np.count_nonzero(fl & 2) >= 2 and (not handlers or o.events.n >= 2), c


@pytest.mark.parametrize("name", rc.FSK4_NAMES)
def test_fsk4_streams(built, name):
    k = rc.fsk4_case(name)
    assert k["x"].shape == (rc.FSK4_B, rc.FSK4_N) and k["y"].shape == (rc.FSK4_B, 2 * rc.FSK4_N)
    for c in range(rc.FSK4_B):
        o = k["oracle"]()
        fresh = o.thresholds()
        out = o.run(k["x"][c])
        assert len(out["sync_pos"]) > 0 and out["fl"][-1] & 1, c
        assert not np.array_equal(_bits(o.thresholds()), _bits(fresh)), c
        o = k["oracle"]()
        out = o.run(k["y"][c])
        assert len(out["sync_pos"]) > 0 and (not k["handlers"] or o.events.n > 0), c
    if name == "dmr":                                   # the two captures print different colour codes (event kind 6)
        cc = []
        for key in ("x", "y"):
            o = k["oracle"]()
            o.run(k[key][0])
            cc.append({e[2] for e in o.events.rows() if e[1] == 6})
        assert cc[0] and cc[1] and cc[0] != cc[1], cc
