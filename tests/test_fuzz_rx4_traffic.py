"""The traffic the protocol fuzz (tests/test_fuzz_rx4_protocols_gpu.py) runs on, judged by the oracle alone: a fuzz whose batches
hold no syncs compares noise with noise.  Every (protocol, case) must hold syncs, hunting and in-frame symbols and a channel that
loses its sync and finds one again; a protocol's eight cases together must reach every pattern row its capture yields, both
polarities, the lock-0 and the longest-lock draws, every kernel shape and both ends of the accepted samples-per-symbol range.  A case
that misses a floor means tests/fuzz_rx4.py's builder is mended - never a skip, never a lower floor."""
import numpy as np
import pytest

import fuzz_rx4 as fz

_STATS = {}


def stats(name, case):
    """the oracle over one case, call by call as the GPU test makes them"""
    if (name, case) not in _STATS:
        c = fz.build(name, case)
        cpu = fz.oracles(c)
        fl = [[] for _ in range(c.B)]
        pats = set()
        for a, b in fz.calls(c):
            for ch in range(c.B):
                o = cpu[ch].run(c.x[ch, a:b], max_sync=fz.max_syncs(b - a, c.sps, c.row.win_len))
                fl[ch].append(o["fl"])
                pats |= set(o["sync_pat"].tolist())
        fl = [np.concatenate(f) for f in fl]
        refound = 0
        for f in fl:
            at = np.flatnonzero(f & 2)
            # a sync, later a hunting symbol that is no sync, later another sync
            refound += any(np.any((f[p + 1:q] & 3) == 0) for p, q in zip(at[:-1], at[1:]))
        _STATS[(name, case)] = dict(c=c, n_sync=sum(int(np.sum((f & 2) != 0)) for f in fl), hunting=sum(int(np.sum((f & 3) == 0)) for f in fl),
                                    inframe=sum(int(np.sum((f & 1) != 0)) for f in fl), refound=refound, pats=pats,
                                    neg={bool(v) for f in fl for v in np.unique(f[(f & 2) != 0] & 4)})
    return _STATS[(name, case)]


@pytest.mark.parametrize("case", range(fz.N_CASES))
@pytest.mark.parametrize("name", fz.PROTOCOLS)
def test_every_case_holds_traffic(name, case):
    s = stats(name, case)
    c = s["c"]
    assert s["n_sync"] >= 3, s["n_sync"]
    assert s["hunting"] >= 1 and s["inframe"] >= 1
    assert s["refound"] >= 1
    kinds = set(c.kinds.values())
    assert {"one-sample", "sub-symbol", "tile", "sync-end"} <= kinds, kinds
    lens = [b - a for a, b in fz.calls(c)]
    assert 1 in lens and any(1 < v < c.sps for v in lens)
    tile = fz.tile_of(c.cpw)            # a call as long as a multiple of the case's staging tile - 1, + 0 or + 1, and a call behind it
    edge = [k for k, v in enumerate(lens) if v >= tile - 1 and min(v % tile, tile - v % tile) <= 1]
    assert edge and any(k + 1 < len(lens) for k in edge), lens
    assert c.tile_calls and all((a, b) in fz.calls(c) for a, b in c.tile_calls)
    assert any(e + 2 in c.cuts for e in c.sync_ends)


@pytest.mark.parametrize("name", fz.PROTOCOLS)
def test_a_protocols_cases_together(name):
    row = fz.ROWS[name]
    all_ = [stats(name, k) for k in range(fz.N_CASES)]
    want = {p for p, _ in fz.scan(name)["rows"]}
    assert set().union(*[s["pats"] for s in all_]) >= want, (want, [s["pats"] for s in all_])
    if row.both:
        assert set().union(*[s["neg"] for s in all_]) == {False, True}
    choice = np.concatenate([s["c"].lock_choice.reshape(-1) for s in all_])
    assert 0 in choice and 3 in choice                                    # the lock-0 draw and the longest lock
    assert {s["c"].cpw for s in all_} == set(fz.CPW)
    assert all(s["c"].B >= 3 for s in all_ if s["c"].cpw >= 8)            # a wide shape with more than lane 0 live
    assert any(s["c"].B % s["c"].cpw for s in all_ if s["c"].cpw > 1)     # a last wavefront that is partly filled
    sps = {s["c"].sps for s in all_}
    assert {5, 10} <= sps if name == "edacs" else {8, 21} <= sps
    assert sum(s["c"].out_rate == 48000 for s in all_) == fz.N_CASES // 2


@pytest.mark.parametrize("name", fz.PROTOCOLS)
def test_densest_streams_stay_below_the_sync_table(name):
    """two accepted syncs lie at least one sync word apart (the hunt restarts with an empty window), so ddn_fsk4_rx_max_syncs =
    max_symbols / win_len + 2 is out of reach; the densest streams of tests/fuzz_rx4.py show how near a call gets"""
    c = fz.build_densest(name)
    cpu = fz.oracles(c)
    total = 0
    for a, b in fz.calls(c):
        for ch in range(c.B):
            o = cpu[ch].run(c.x[ch, a:b], max_sync=fz.max_syncs(b - a, c.sps, c.row.win_len))
            at = o["sync_pos"]
            assert len(at) <= (len(o["sym"]) - 1) // c.row.win_len + 1 < fz.max_syncs(b - a, c.sps, c.row.win_len)
            assert len(at) < 2 or np.diff(at).min() >= c.row.win_len
            total += len(at)
    assert total >= 20 * c.B, total
