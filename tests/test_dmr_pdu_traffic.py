"""CPU: the generated DMR PDU traffic (tests/dmrpdugen.traffic) holds every case the GPU tests compare on, counted through the
restatement alone (tests/dmr_pdu.py) - so a GPU test that finds "every output equal" cannot have passed over an empty list."""
import numpy as np
import pytest

import dmr_pdu as dp
import dmrpdugen as gen


@pytest.fixture(scope="module")
def run():
    items, marks, notes = gen.traffic(0)
    bursts = gen.fec_bursts(items)
    outs, pdus, _ = dp.walk(bursts, marks)
    return items, marks, notes, bursts, outs, pdus


def _pdu_at(pdus, k):
    hit = [p for p in pdus if p["burst"] == k]
    assert len(hit) == 1, k
    return hit[0]


def test_every_kind_of_pdu_completes(run):
    items, _, notes, bursts, outs, pdus = run

    def data(name, back=0):
        return _pdu_at(pdus, notes[name] - back)
    # (an interleaved pair ends on the second slot's last item unless the first is longer)
    p = data("unconf12|conf34")
    assert (p["kind"], p["slot"], p["confirmed"], p["n"], p["crc"], p["dpf"]) == (dp.KIND_DATA, 1, 1, 64, 1, 3)
    assert p["valid"][1:5].all()
    q = [x for x in pdus if x["slot"] == 0 and x["burst"] < notes["unconf12|conf34"]][0]
    assert (q["kind"], q["confirmed"], q["n"], q["crc"], q["dpf"]) == (dp.KIND_DATA, 0, 36, 1, 2)
    lens = sorted((x["slot"], x["confirmed"], x["n"], x["crc"]) for x in pdus if x["burst"] <= notes["unconf34|unconf1"])
    assert lens == sorted([(0, 0, 36, 1), (1, 1, 64, 1), (0, 1, 30, 1), (1, 1, 44, 1), (0, 0, 36, 1), (1, 0, 48, 1)])
    # the MNIS header: offset 12 for the CRC walk, ten bytes in front, the CRC32 waived
    m = [x for x in pdus if x["p_head"] == 1]
    assert len(m) == 1 and (m[0]["n"], m[0]["dpf"], m[0]["sap"], m[0]["crc"], m[0]["slot"]) == (10 + 36, 15, 1, 1, 0)
    v = [x for x in pdus if x["dpf"] == 15 and x["p_head"] == 0]
    assert len(v) == 1 and (v[0]["n"], v[0]["sap"], v[0]["crc"], v[0]["blocks"]) == (54, 4, 1, 3)
    mb = [x for x in pdus if x["kind"] == dp.KIND_MBC]
    assert sorted((x["n"], x["hdr_crc"], x["blk_crc"]) for x in mb) == [(24, 1, 0), (36, 1, 1), (48, 1, 1)]
    ud = [x for x in pdus if x["kind"] == dp.KIND_UDT]
    assert [(x["n"], x["crc"], x["blocks"]) for x in ud] == [(36, 1, 2), (36, 1, 3)]          # fixed count, reserved count (CRC-terminated)
    sd = [x for x in pdus if x["dpf"] == 13]
    assert len(sd) == 1 and (sd[0]["confirmed"], sd[0]["n"], sd[0]["crc"], sd[0]["sap"]) == (1, 20, 1, 10)


def test_the_failures_are_there(run):
    items, marks, notes, bursts, outs, pdus = run
    st = [o["status"] for o in outs]
    bad = [x for x in pdus if x["kind"] == dp.KIND_DATA and x["crc"] == 0]
    assert len(bad) >= 1 and any(x["burst"] == notes["bad_crc32|bad_crc16"] for x in bad)
    assert st.count(dp.ST_HDR_CRC) == 1 and st[notes["header_crc"] - 2] == dp.ST_HDR_CRC
    assert st.count(dp.ST_HDR_FEC) == 1
    assert st.count(dp.ST_SEQ_ERR) == 2 and st[notes["seq_error"] - 1] == dp.ST_SEQ_ERR      # (and the block behind the bad CRC9)
    k = notes["seq_error"] - 1
    assert (outs[k]["conf"], outs[k]["dbsn"], outs[k]["crc"]) == (1, 9, 1) and outs[k + 1]["conf"] == 0
    k = notes["bad_crc9"] - 1
    assert (outs[k]["conf"], outs[k]["crc"], outs[k]["status"]) == (1, 0, dp.ST_FILED)
    assert st.count(dp.ST_TERMINATOR) >= 1 and not any(p["burst"] == notes["terminated"] for p in pdus)
    assert st.count(dp.ST_MBC_HEADER) == 3


def test_resets_cut_a_pdu_and_the_next_one_completes(run):
    items, marks, notes, bursts, outs, pdus = run
    assert [kind for _, kind in marks] == [0, 1]
    for name, after in (("reset_mid", "after_reset"), ("loss_mid", "after_loss")):
        cut = notes[name]
        assert outs[cut]["status"] == dp.ST_FILED and outs[cut]["counter"] == 1          # the PDU was under way
        assert outs[cut + 1]["counter"] == 1 and outs[cut + 1]["status"] == dp.ST_FILED  # ... and its next block met the reset state
        done = [p for p in pdus if cut < p["burst"] <= notes[after]]
        assert len(done) == 1 and done[0]["burst"] == notes[after] and done[0]["crc"] == 1
    # carrier loss leaves data_conf_data standing, dmr_reset_blocks() clears it
    assert outs[notes["loss_mid"] + 1]["conf"] == 1 and outs[notes["reset_mid"] + 1]["conf"] == 0


def test_both_time_slots_carry_pdus_side_by_side(run):
    items, _, notes, bursts, outs, pdus = run
    k = notes["unconf12|conf34"]
    slots = [it["slot"] for it in items[:k + 1]]
    assert slots[:8] == [0, 1] * 4
    a, b = [p for p in pdus if p["burst"] <= k]
    assert {a["slot"], b["slot"]} == {0, 1} and not np.array_equal(a["bytes"], b["bytes"])
    assert a["burst"] > 1 and b["burst"] > a["burst"]            # the second header lies inside the first PDU


def test_marks_from_the_loop_events():
    """dp.marks_of: resets in event order among the dispatched bursts, carrier loss at the 1800th quiet symbol"""
    ev = [(100, 5, 1, 7, 6), (143, 6, 7, 0, 0), (300, 5, 0, -1, -1), (500, 5, 1, 7, 3 | 1 << 8), (700, 5, 1, 7, 7), (743, 6, 7, 0, 1),
          (900, 8, 0, 1, 0), (950, 8, 1, 1, 1), (1000, 5, 0, -2, -1)]
    fl = np.ones(6000, np.uint8)
    fl[1100:2899] = 0                       # 1799 quiet symbols: none
    fl[3000:4801] = 0                       # 1801: one, at 4799
    assert dp.marks_of(ev, fl, [143, 743]) == [(1, 0), (1, 0), (2, 0), (2, 0), (2, 1)]
    fl[:] = 0
    assert [m for m in dp.marks_of([], fl, [1798, 1800, 3600]) if m[1] == 1] == [(1, 1), (2, 1), (3, 1)]


def test_the_stream_for_the_chain_holds_its_cases(built):
    """dmrpdugen.air_batch() through the oracle front end and receive loop, one call: what the chain test compares on is there"""
    import chain_fsk4_stream as cs
    import rx4
    x = gen.air_batch()
    for c in range(x.shape[0]):
        o = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, rf_mod=2, handler=1))
        w = o.run(cs.front_end_disc(x[c], x.shape[1], 2), max_sync=4096)
        pos, bursts, marks, outs, pdus = dp.stream_reference(w, o.events.rows())
        st = [o["status"] for o in outs]
        assert len(bursts) >= 50 and {b["slot"] for b in bursts} == {0, 1}
        kinds = sorted((p["kind"], p["confirmed"], p["n"], p["crc"]) for p in pdus)
        # unconfirmed 1/2 (36), confirmed 3/4 (48), confirmed rate 1 (44), confirmed 1/2 with a bad CRC32 (20), the MNIS header (34)
        for want in ((dp.KIND_DATA, 0, 36, 1), (dp.KIND_DATA, 1, 48, 1), (dp.KIND_DATA, 1, 44, 1), (dp.KIND_DATA, 1, 20, 0), (dp.KIND_DATA, 0, 34, 1),
                     (dp.KIND_MBC, 0, 36, 1), (dp.KIND_UDT, 0, 36, 1)):
            assert want in kinds, (c, want, kinds)
        assert any(p["p_head"] == 1 for p in pdus)
        # UDT: the fixed count (two appended blocks announced) and the reserved count (three announced, closed by its CRC16 after two)
        assert sorted((p["blocks"], p["n"], p["crc"]) for p in pdus if p["kind"] == dp.KIND_UDT) == [(2, 36, 1), (3, 36, 1)], c
        assert sorted((p["n"], p["crc"]) for p in pdus if p["kind"] == dp.KIND_MBC) == [(36, 1), (48, 1)], c
        assert st.count(dp.ST_SEQ_ERR) == 1 and st.count(dp.ST_HDR_CRC) == 1
        # a reset from a failed slot type and one from carrier loss, each with a PDU under way on a time slot
        inside = [(b, k) for b, k in marks if 0 < b < len(outs) and any(o["counter"] > 1 for o in outs[max(0, b - 3):b])]
        assert {k for _, k in inside} == {0, 1}, (c, marks)
        assert len(pdus) >= 11
