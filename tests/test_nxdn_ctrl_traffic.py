"""CPU: the generated NXDN streams hold what the GPU tests compare (tests/test_nxdn_ctrl_gpu.py, tests/test_nxdn_ctrl_chain_gpu.py), so
that none of them can pass on an empty list.  The generated batch (tests/nxdngen.air_batch: three channels - as sent, delayed,
starting later) through the oracle loop and the restatement yields on every channel the floors below; the inputs of the direct calls
hold frames the hard retry rescues and frames that fail both decodes."""
import numpy as np
import pytest

import chain_fsk4_stream as cs
import nxdn_ctrl as nc
import nxdngen as gen

_W = {}


def stream(which, c):
    if (which, c) not in _W:
        x = gen.air_batch(which)
        _W[(which, c)] = nc.stream_reference(cs.nxdn_oracle_stream(x[c], x.shape[1], which))
    return _W[(which, c)]


@pytest.mark.parametrize("c", [0, 1, 2])
def test_floors_of_the_generated_batch(built, c):
    ref = stream("nxdn96", c)
    fr, wk = [f for _, f, _ in ref], [w for _, _, w in ref]
    n = lambda kind, ok: sum(f["kind"] == kind and bool(f["crc_ok"]) == ok for f in fr)
    assert n(nc.KIND_CAC, True) >= 12 and n(nc.KIND_CAC, False) >= 2
    assert n(nc.KIND_FACCH2, True) >= 4 and n(nc.KIND_UDCH, True) >= 4
    assert sum(w["msg_status"] == 1 and w["sacch_status"] == 1 for w in wk) >= 3          # delivered SACCH messages
    assert sum(w["msg_status"] == 2 for w in wk) >= 1                                      # completed, a segment was bad
    assert sum(w["sacch_status"] == 1 and not w["seq_ok"] for w in wk) >= 1               # a good segment out of sequence
    assert sum(w["sacch_status"] in (3, 4) for w in wk) >= 1                               # non-superframe SACCH
    # a LICH with good parity off the profile table between two segments of one superframe: the message behind it completes undelivered
    miss = [k for k, f in enumerate(fr) if f["parity"] and f["lich"] not in nc.LICH_PROFILE]
    def lands_between_segments(k):
        before = [w for w in wk[:k] if w["sacch_status"]]
        after = [w for w in wk[k:] if w["sacch_status"] == 1 and w["pf"] == 3]
        return bool(before and after) and before[-1]["sacch_status"] == 1 and before[-1]["pf"] in (0, 1, 2) and after[0]["msg_status"] == 2

    assert any(lands_between_segments(k) for k in miss)
    # a FACCH2 frame between two SACCH segments: its part_of_frame write decides the next seq_ok
    between = [k for k in range(1, len(fr) - 1) if fr[k]["kind"] == nc.KIND_FACCH2 and wk[k - 1]["sacch_status"] == 1 and wk[k + 1]["sacch_status"] == 1]
    assert between
    for k in between:
        want_part = (wk[k]["pf"] + 1) % 4
        assert bool(wk[k + 1]["seq_ok"]) == (wk[k + 1]["pf"] in (0, want_part)), k
    assert any(wk[k]["pf"] != wk[k - 1]["pf"] for k in between)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_floors_of_the_shorter_nxdn48_stream(built, c):
    ref = stream("nxdn48", c)
    fr, wk = [f for _, f, _ in ref], [w for _, _, w in ref]
    assert sum(f["kind"] == nc.KIND_CAC and f["crc_ok"] for f in fr) >= 8 and sum(f["kind"] >= 2 and f["crc_ok"] for f in fr) >= 6
    assert sum(w["msg_status"] == 1 for w in wk) >= 2


def test_the_direct_inputs_hold_retry_and_failure(built):
    """in the records of the direct GPU test at least 3 frames are taken by the hard retry with a good CRC and at least 2 fail both
    decodes; clean dibits under reliabilities of 0 are what the retry rescues (the soft decoder has nothing to go on), and some frames
    are the soft decoder's"""
    rescued = failed = soft = quiet = 0
    for name in gen.DIRECT_CASES:
        d = gen.direct_case(name)
        B, S = d["sync_pos"].shape
        for c in range(B):
            for k in range(int(d["n_sync"][c])):
                f = nc.slot_frame(d["rec"], d["counts"], c, int(d["sync_pos"][c, k]))
                if f is None:
                    continue
                fr = nc.decode_frame(*f)
                if not fr["kind"]:
                    continue
                rescued += fr["fallback"] and fr["crc_ok"]
                failed += not fr["crc_ok"]
                soft += not fr["fallback"]
                if not f[1].any():
                    quiet += 1
                    assert fr["fallback"] == 1
    assert rescued >= 3 and failed >= 2 and soft >= 6 and quiet >= 3, (rescued, failed, soft, quiet)
    d = gen.direct_case("sparse")
    f = nc.slot_frame(d["rec"], d["counts"], 0, int(d["sync_pos"][0, 20]))
    assert not f[1].any() and nc.decode_frame(*f)["crc_ok"] == 1 and nc.decode_frame(*f)["fallback"] == 1
