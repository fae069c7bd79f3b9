"""CPU: floors under the traffic of the DMR MS chain test (tests/dmrmsgen.air_batch through the pinned front end and the oracle loop,
tests/dmr_ms.chain_reference), by the restatement alone - so that tests/test_dmr_ms_chain_gpu.py cannot pass on empty traffic.
No floor for a failed TACT: Hamming(7,4) refuses no word (tests/test_dmr_ms.py::test_hamming_7_4_refuses_nothing)."""
import numpy as np
import pytest

import dmr_ms
import dmrmsgen as gen

SIZES = (2000, 30, 10)          # samples per call: 200, 3 and 1 symbols


def test_the_stream_is_about_two_seconds(built):
    x = gen.air_batch()
    assert x.shape[0] == 8 and 1.9 <= x.shape[1] / 48000 <= 2.3 and all(x.shape[1] % n == 0 for n in SIZES)


@pytest.mark.parametrize("c", range(8))
def test_every_channel_carries_every_kind(built, c):
    x = gen.air_batch()
    r = dmr_ms.chain_reference(x, c, x.shape[1])
    vcs = [v["vc"] for v in r["voice"]]
    units = sum(vcs[i:i + 6] == [1, 2, 3, 4, 5, 6] for i in range(len(vcs)))
    assert units >= 2 and sum(l["ok"] and not l["errs"] for l in r["lc"]) >= 1 and any(not l["ok"] for l in r["lc"])
    types = [b["fec"]["type"] for b in r["data"] if b["status"] == 0]
    for ty in (1, 2, 3, 6, 7, 8, 10):
        assert ty in types, ty
    assert any(b["pat"] == 5 and b["slot"] == 1 and b["status"] == 0 for b in r["data"])
    assert any(b["pat"] == 4 and b["slot"] == 0 and b["status"] == 0 for b in r["data"])
    assert any(b["status"] == 2 for b in r["data"]) and any(v["emb_ok"] == 0 for v in r["voice"])
    assert any(b["status"] == 0 and b["fec"]["type"] == 8 and b["fec"]["confirmed_crc"] for b in r["data"])
    assert {v["emb_cc"] for v in r["voice"] if v["emb_ok"] == 1} == {5, 9} and r["cc"] == 5


@pytest.mark.parametrize("n", SIZES)
def test_bursts_straddle_call_boundaries(built, n):
    """at every call size: a burst of a unit's cycle and a burst with a hand-over (data or bootstrap) whose first and last symbols lie
    in different calls"""
    x = gen.air_batch()
    r = dmr_ms.chain_reference(x, 0, n)
    call_of = lambda p: int(np.searchsorted(r["held"], p, side="right"))
    cyc = [v for v in r["voice"] if v["vc"] > 1 and call_of(v["start"]) != call_of(v["start"] + 143)]
    hand = [b for b in r["data"] + [v for v in r["voice"] if v["vc"] == 1] if call_of(b["start"]) != call_of(b["start"] + 143)]
    assert len(cyc) >= 1 and len(hand) >= 1, (len(cyc), len(hand))
