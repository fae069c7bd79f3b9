"""CPU: the restatement of the DMR PDU layer (tests/dmr_pdu.py) and the generator's blocks (tests/dmrpdugen.py) against vectors taken
as data from the reference's own DMR tests (tests/golden/dmr_pdu_vectors.json, written by tests/golden/make_golden_dmr_pdu.py)."""
import json
import os

import numpy as np
import pytest

import dmr_pdu as dp
import dmrpdugen as gen


@pytest.fixture(scope="module")
def vec():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dmr_pdu_vectors.json")))


def test_profile_table(vec):
    """dmr_dburst_profile_resolve(): every row of the reference's expected table for data types 0 .. 11"""
    rows = [r for r in vec["profiles"] if r["databurst"] <= 11]
    assert len(rows) == 17
    for r in rows:
        got = dp.profile(r["databurst"], r["confirmed"], r["header_format"])
        want = dict(crcmask=r["crcmask"], crclen=r["crclen"], pdu_len=r["pdu_len"], pdu_start=r["pdu_start"], udt=int("DMR_DBURST_F_UDT" in r["flags"]))
        assert got == want, (r, got)


def test_walk_files_what_the_profile_says(vec):
    """a block of every rate, confirmed and not, moves data_byte_ctr by the profile's PDU length and leaves out pdu_start bytes"""
    rng = np.random.default_rng(1)
    for r in vec["profiles"]:
        if r["databurst"] not in (7, 8, 10) or r["header_format"] == 0:
            continue
        conf = r["confirmed"]
        chunk = rng.integers(0, 256, gen.BLOCK_LEN[(r["databurst"], conf)])
        items = [gen.header(0, 3 if conf else 2, 5), gen.block(0, r["databurst"], conf, chunk)]
        outs, pdus, w = dp.walk(gen.fec_bursts(items))
        assert w.s[0].byte_ctr == r["pdu_len"] and np.array_equal(w.s[0].sf[:r["pdu_len"]], chunk)
        assert outs[1]["crc"] == 1 and outs[1]["conf"] == conf


def test_confirmed_crc9_spans(vec):
    """the reference's three confirmed blocks: the CRC9 over the payload bits then the DBSN, masked per rate, checks; one flipped
    payload bit and it does not"""
    for v in vec["crc9"]:
        chunk = np.packbits(np.array(v["payload"], np.uint8))
        assert gen.CRC9_MASK[v["rate"]] == v["mask"]
        # the value the reference's own ComputeCrc9Bit gave for the span (recorded), against the generator's and the walk's CRC9
        import p25gen
        assert p25gen.crc9(v["payload"] + [(v["dbsn"] >> (6 - i)) & 1 for i in range(7)]) == v["crc9_ref"]
        for flip in (False, True):
            it = gen.block(0, v["rate"], True, chunk, dbsn=v["dbsn"])
            if flip:
                key = {7: "bits96", 8: "bytes18", 10: "info196"}[v["rate"]]
                if v["rate"] == 8:
                    b = np.unpackbits(it[key])
                    b[16 + v["flip"]] ^= 1
                    it[key] = np.packbits(b)
                else:
                    it[key][16 + v["flip"]] ^= 1
            outs, _, w = dp.walk(gen.fec_bursts([gen.header(0, 3, 5), it]))
            assert (outs[1]["conf"], outs[1]["dbsn"], outs[1]["crc"]) == (1, v["dbsn"], 0 if flip else 1), (v["rate"], flip)
            assert w.s[0].crc_valid[1] == (0 if flip else 1)


def _seeded(seed, **kw):
    w = dp.Walk()
    s = w.s[0]
    s.hvalid, s.counter, s.blocks, s.conf, s.hfmt, s.sap = (seed["header_valid"], seed["block_counter"], seed["header_blocks"], seed["conf"],
                                                          seed["header_format"], seed["sap"])
    for k, v in kw.items():
        setattr(s, k, v)
    return w


def test_type1_append_saturates(vec):
    """dmr_block_type1_append_bytes(): a normal append, one that straddles the row's end, a counter already past it, and 64 blocks
    in a row that never complete"""
    t = vec["type1_bounds"]
    assert t["cap"] == dp.ROW
    block = [0x40 + i for i in range(24)]
    for c in t["cases"]:
        if c["byte_ctr"] is None:
            w = _seeded(t["seed"])
            for _ in range(c["repeat"]):
                w.s[0].counter, w.s[0].blocks, w.s[0].hvalid = 1, 9, 1
                w._assemble(0, block, c["block_len"], 1)
                assert w.s[0].byte_ctr <= c["want_max"]
            continue
        w = _seeded(t["seed"], byte_ctr=c["byte_ctr"])
        w._assemble(0, block, c["block_len"], 1)
        assert w.s[0].byte_ctr == c["want"], c


def test_type2_stays_inside_its_buffers(vec):
    """the UDT block counts the reference seeds (4, 127, 6, 7): the assembler completes or files without touching anything past the row"""
    t = vec["type2_bounds"]
    block = [0xC0 + i for i in range(24)]
    for n in t["udt_blocks"]:
        w = dp.Walk()
        s = w.s[0]
        s.hvalid, s.blocks, s.counter, s.hfmt = 1, n, n, 0
        s.crc_valid[0] = 1
        s.sf[:] = [(0x5A + (i & 0x0F)) & 0xFF for i in range(dp.ROW)]
        w._assemble(0, block, 12, 3)
        assert len(s.sf) == dp.ROW and len(w.pdus) == 1 and w.pdus[0]["kind"] == dp.KIND_UDT and w.pdus[0]["n"] == min(12 * (n + 1), dp.ROW)


def test_crc32_of_the_generator_and_the_restatement_agree_on_odd_cases():
    """the generator's byte-wise CRC32 trailer against the restatement's bit-serial walk: lengths around a block, with the MNIS lead"""
    rng = np.random.default_rng(2)
    for n in (4, 6, 12, 22, 36, 46, 3048):
        body = [int(x) for x in rng.integers(0, 256, n - 4)]
        row = body + gen.crc32_trailer(body)
        bits = dp.type1_crc_bits(row, 12, n, 0, 0)
        assert dp.crc32_bits(bits[:8 * n - 32]) == int.from_bytes(bytes(row[-4:]), "big"), n


FIELDS = ("hfmt", "sap", "blocks", "counter", "conf", "hvalid", "p_head", "poc", "byte_ctr", "dbsn_have", "dbsn_exp", "udt_res", "src", "tgt", "gi")


def _state_of(w):
    out = []
    for s in w.s:
        d = {k: int(getattr(s, k)) for k in FIELDS}
        d["crc_valid0"] = int(s.crc_valid[0])
        d["sf"] = bytes(s.sf[:96]).hex()
        out.append(d)
    return out


def test_sequences_recorded_from_the_reference(vec):
    """every call of the recorded runs of the reference's dmr_dheader() / dmr_block_assembler() / dmr_reset_blocks() under the default
    options, replayed through the restatement: both slots' fields and the head of the row after every call, and for every block whether
    a PDU completed and with which verdict - a type 1 PDU or a UDT message is dispatched in strict mode exactly when its CRC checks (the
    MNIS header waives it), an MBC hands its verdict to dmr_cspdu().  The CRC32 trailers in these rows were made by the reference's
    ComputeCrc32Bit, the CRC16s by its dsd_crc_ccitt16_bits: they pin the byte order, and that confirmed blocks take part whole."""
    names = []
    w = None
    seen = dict(data_ok=0, data_bad=0, udt=0, mbc=0, waived=0)
    for s in vec["sequences"]:
        if s["step"] == 0:
            w = dp.Walk()
            names.append(s["scenario"])
        slot, data = s["slot"], np.frombuffer(bytes.fromhex(s["input"]), np.uint8)
        before = len(w.pdus)
        if s["op"] == "seed":
            for q in range(2):
                for k in FIELDS:
                    setattr(w.s[q], k, s["state"][q][k])
                w.s[q].crc_valid[0] = s["state"][q]["crc_valid0"]
                w.s[q].sf[:96] = np.frombuffer(bytes.fromhex(s["state"][q]["sf"]), np.uint8)
        elif s["op"] == "header":
            w._dheader(slot, data, s["a"], s["b"])
        elif s["op"] == "block":
            w._assemble(slot, data, s["a"], s["b"])
        else:
            assert s["op"] == "reset"
            w.reset_blocks()
        assert _state_of(w) == s["state"], (s["scenario"], s["step"], s["op"])
        if s["op"] != "block":
            continue
        done = w.pdus[before:]
        if not done:
            assert s["dispatched"] == 0 and s["cspdu"] == 0, (s["scenario"], s["step"])
            continue
        assert len(done) == 1
        p = done[0]
        if p["kind"] == dp.KIND_MBC:
            assert (s["cspdu"], s["cspdu_crc"]) == (1, p["crc"]), (s["scenario"], s["step"])
            seen["mbc"] += 1
        else:
            assert int(s["dispatched"] > 0) == p["crc"], (s["scenario"], s["step"], p["crc"])
            seen["udt" if p["kind"] == dp.KIND_UDT else ("data_ok" if p["crc"] else "data_bad")] += 1
            seen["waived"] += int(p["p_head"] == 1)
    assert len(names) == len(set(names)) >= 20
    assert seen["data_ok"] >= 11 and seen["data_bad"] == 1 and seen["udt"] == 1 and seen["mbc"] == 1 and seen["waived"] == 1, seen
