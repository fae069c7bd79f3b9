"""The traffic the short-call chain tests (tests/test_chain_fsk4_short_calls_gpu.py) run on, judged by the oracle alone: a chain that
decodes nothing equals a reference that holds nothing.  For every (protocol, call size, stream) of tests/chain_fsk4_stream.py the
whole-stream reference must hold at least six valid units per channel, units whose sync waits in the carried list, new-record counts on
both sides of the carry at the at-the-carry size, voice and DMR data traffic where the case is about them - and never more waiting or
decoded syncs than the chain has places for (the cases are about correctness, not about the drop counter).  The plain, voice, DMR
handler and mixed-chain streams are all held to the same floors (holds_the_floors).

How long a sync waits: a sync at stream position P is accepted in the call k whose records reach P and decoded in the first call j whose
records reach P + T (T = the carry).  j - k >= 2 is asked wherever a call brings fewer than T records (below the carry, tiny, D-STAR at
one demodulator block).  Where a call brings T records or more (at the carry, one block for the other seven) P + T lies in call k or
k + 1 by arithmetic, so no sync can wait two calls; there the floor is j - k >= 1: a sync decoded out of the carried list."""
import numpy as np
import pytest

import chain_fsk4_stream as cs

_STATS = {}


def stats(proto, kind, n):
    key = (proto, kind, n)
    if key not in _STATS:
        x = cs.stream(proto, kind)
        T = cs.ROWS[proto]["T"]
        want = cs.oracle_of(proto, kind, n)
        per = []
        for c in range(x.shape[0]):
            every, valid = cs.sync_positions(proto, want[c])
            held = cs.held_after_calls(proto, x[c], n)
            every, valid = np.array(every, np.int64), np.array(valid, np.int64)
            acc = lambda p: np.searchsorted(held, p, side="right")                 # the call that brings record p
            wait = acc(valid + T) - acc(valid)
            k_acc, k_dec = acc(every), acc(every + T)
            calls = len(held)
            waiting = max([int(np.sum((k_acc <= j) & (k_dec > j))) for j in range(calls)] + [0])
            decoded = max([int(np.sum(k_dec == j)) for j in range(calls + 1)] + [0])
            wait = wait[valid + T < held[-1]]               # (what the flush decodes waited for the stream's end, not for records)
            per.append(dict(valid=len(valid), wait=wait, new=np.diff(np.concatenate([[0], held])), waiting=waiting, decoded=decoded))
        _STATS[key] = per
    return _STATS[key]


def holds_the_floors(proto, kind, n):
    """the floors every (protocol, call size, stream) meets: 3 or 4 channels of six valid units or more, three units or more whose sync
    waits, never more waiting or decoded syncs than the chain has places for -> the per-channel figures"""
    row = cs.ROWS[proto]
    per = stats(proto, kind, n)
    assert len(per) in (3, 4)
    assert all(s["valid"] >= 6 for s in per), [s["valid"] for s in per]
    short = n < row["sps"] * row["T"]              # a call brings fewer records than the carry holds
    assert sum(int(np.sum(s["wait"] >= (2 if short else 1))) for s in per) >= 3
    myd, myc = cs.decode_slots(proto, n)
    assert all(s["waiting"] <= myc and s["decoded"] <= myd for s in per), [(s["waiting"], s["decoded"]) for s in per]
    return per


@pytest.mark.parametrize("proto,size", cs.cases())
def test_every_short_call_case_holds_traffic(proto, size):
    n = cs.call_size(proto, size)
    kind = "tiny" if size == "tiny" else "plain"
    row = cs.ROWS[proto]
    per = holds_the_floors(proto, kind, n)
    if size == "below":
        assert all(np.all(s["wait"] >= 2) for s in per)        # every sync decoded in a call waits
    if size == "at":
        seen = set().union(*[set(s["new"].tolist()) for s in per]) & {row["T"] - 1, row["T"], row["T"] + 1}
        assert len(seen) >= 2, seen
    if proto == "m17":      # the LICH assembly buffer is carried: every channel completes an LSF from its chunks
        assert all(sum("lich_lsf30" in f for f in w[1]) >= 1 for w in cs.oracle_of(proto, kind, n))
    if proto == "ysf" and size != "tiny":   # ysf.last is carried: frames of a known type on every channel
        assert all(sum(f["err"] == 0 for f in w[2]) >= 6 for w in cs.oracle_of(proto, kind, n))


@pytest.mark.parametrize("proto", cs.VOICE)
def test_every_voice_case_synthesises(proto):
    """vocoder = 1 at the below-the-carry size: at least 20 synthesised frames on every talk path that carries voice, and one such path
    per channel (YSF: the AMBE path - V/D modes 1 and 2 - and the IMBE path - full-rate - of every channel)"""
    n = cs.call_size(proto, "below")
    want = cs.oracle_of(proto, "voice", n)
    per = holds_the_floors(proto, "voice", n)
    assert all(np.sum(s["wait"] >= 2) >= 3 for s in per)
    for c, w in enumerate(want):
        if proto == "dmr":
            paths = [3 * sum(1 for e in w["voice"] if e[4] == slot) for slot in range(2)]
            assert max(paths) >= 20 and all(v == 0 or v >= 20 for v in paths), (c, paths)
        elif proto == "nxdn48":
            assert len(cs.nxdn_voice_plan(w)) >= 20, c
        elif proto == "ysf":
            plan = cs.ysf_voice_plan(w)
            assert sum(p[1] for p in plan["a"]) >= 20 and sum(p[1] for p in plan["i"]) >= 20, c
            kinds = {f["payload"]["kind"] for f in w[2] if f["payload"] is not None}
            assert {1, 2, 4} <= kinds, (c, kinds)
        else:
            assert len(cs.dpmr_voice_plan(w)) >= 20, c


@pytest.mark.parametrize("size", cs.HANDLER_SIZES)
def test_the_dmr_handler_case_holds_every_kind(size):
    """link control bursts, rate 3/4 confirmed and unconfirmed, embedded link control - and bursts whose decision falls in a later call
    than their sync"""
    n = cs.call_size("dmr", size)
    want = cs.oracle_of("dmr", "handlers", n)
    holds_the_floors("dmr", "handlers", n)
    data = [x for w in want for _, _, x in w["data"]]
    assert sum(x["type"] in (1, 2) and (x["crc"] & 1) for x in data) >= 1
    assert sum(x["type"] == 8 and x["confirmed_crc"] == 1 for x in data) >= 1
    assert sum(x["type"] == 8 and x["confirmed_crc"] == 0 for x in data) >= 1
    assert sum(len(w["lcs"][0]) + len(w["lcs"][1]) for w in want) >= 1
    # a data burst found by the sync search: its decision comes 54 symbols behind its sync
    split = 0
    for c, w in enumerate(want):
        held = cs.held_after_calls("dmr", cs.stream("dmr", "handlers")[c], n)
        syncs = set(int(p) for p in w["w"]["sync_pos"])
        for pos, _, _ in w["data"]:
            if pos - 54 in syncs:
                split += int(np.searchsorted(held, pos, side="right") != np.searchsorted(held, pos - 54, side="right"))
    assert split >= 1


@pytest.mark.parametrize("proto", ["dmr", "nxdn48"])
def test_the_mixed_chain_groups_hold_traffic(proto):
    """the DMR and NXDN48 groups of the mixed-chain case (the start of the plain streams, in calls of one demodulator block)"""
    holds_the_floors(proto, "mixed", cs.MIXED_N)
