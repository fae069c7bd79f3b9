"""GPU: ddn_dmr_pdu_walk_batch / ddn_dmr_pdu_marks_batch (include/ddn_fsk4.h, ddn_dmr_pdu.hip) on made-up burst lists against the
restatement (tests/dmr_pdu.py): every per-burst and per-PDU output, the state carried from call to call."""
import ctypes as C

import numpy as np
import pytest

import ddn
import dmr_pdu as dp
import dmrpdugen as gen

pytestmark = pytest.mark.gpu


class Dev:
    """device copies that live as long as the object"""

    def __init__(self):
        self.l = ddn.lib()
        self.ptrs = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.l.ddn_device_alloc(max(a.nbytes, 4), C.byref(p)) == 0
        if a.nbytes:
            assert self.l.ddn_device_upload(p, a.ctypes.data, a.nbytes) == 0
        self.ptrs.append(p)
        return p

    def down(self, p, dtype, shape):
        a = np.zeros(shape, dtype)
        assert self.l.ddn_device_download(a.ctypes.data, p, a.nbytes) == 0
        return a

    def close(self):
        for p in self.ptrs:
            self.l.ddn_device_free(p)
        self.ptrs = []


def pack(chans, nb, nm):
    """[(bursts, marks)] per channel -> the input arrays of ddn_dmr_pdu_input"""
    B = len(chans)
    a = dict(n=np.zeros(B, np.int32), slot=np.zeros((B, nb), np.uint8), type=np.full((B, nb), 0xFF, np.uint8), by=np.zeros((B, nb, 12), np.uint8),
             info=np.zeros((B, nb, 196), np.uint8), errs=np.zeros((B, nb), np.uint32), crc=np.zeros((B, nb), np.uint8),
             un=np.zeros((B, nb, 18), np.uint8), pool=np.full((B, nb, 34, 24), 0xEE, np.uint8), pn=np.zeros((B, nb), np.int32),
             nr=np.zeros(B, np.int32), rb=np.zeros((B, nm), np.int32), nl=np.zeros(B, np.int32), lb=np.zeros((B, nm), np.int32))
    for c, (bursts, marks) in enumerate(chans):
        assert len(bursts) <= nb
        a["n"][c] = len(bursts)
        for k, x in enumerate(bursts):
            a["slot"][c, k], a["type"][c, k], a["by"][c, k], a["info"][c, k] = x["slot"], x["type"], x["bytes12"], x["info"]
            a["errs"][c, k], a["crc"][c, k], a["un"][c, k] = x["errs"], x["crc"], x["unconfirmed"]
            a["pn"][c, k] = len(x["pool"])
            for j, (b18, metric, ok, dbsn) in enumerate(x["pool"]):
                a["pool"][c, k, j, :4] = np.array([metric], np.int32).view(np.uint8)
                a["pool"][c, k, j, 4:22], a["pool"][c, k, j, 22], a["pool"][c, k, j, 23] = b18, ok, dbsn
        r = [b for b, kind in marks if kind == 0]
        lo = [b for b, kind in marks if kind == 1]
        assert len(r) <= nm and len(lo) <= nm
        a["nr"][c], a["nl"][c] = len(r), len(lo)
        a["rb"][c, :len(r)], a["lb"][c, :len(lo)] = r, lo
    return a


class Walker:
    """the state block of B channels and one call after another through ddn_dmr_pdu_walk_batch"""

    def __init__(self, B, P=4):
        self.d, self.B, self.P = Dev(), B, P
        self.state = self.d.up(np.zeros(B * ddn.lib().ddn_dmr_pdu_state_bytes(), np.uint8))

    def call(self, chans, nb=None, nm=8):
        d, B, P = self.d, self.B, self.P
        nb = nb or max(1, max(len(b) for b, _ in chans))
        a = pack(chans, nb, nm)
        keep = len(d.ptrs)
        inp = ddn.DmrPduInput(B, nb, nm, *[d.up(a[k]) for k in ("n", "slot", "type", "by", "info", "errs", "crc", "un", "pool", "pn", "nr", "rb", "nl", "lb")])
        shapes = [("conf", np.uint8, (B, nb)), ("counter", np.int32, (B, nb)), ("crc", np.uint8, (B, nb)), ("dbsn", np.uint8, (B, nb)),
                  ("pick", np.int32, (B, nb)), ("status", np.uint8, (B, nb)), ("n_pdus", np.int32, (B,)), ("kind", np.uint8, (B, P)),
                  ("slot", np.uint8, (B, P)), ("burst", np.int32, (B, P)), ("len", np.int32, (B, P)), ("bytes", np.uint8, (B, P, 3072)),
                  ("crc4", np.uint8, (B, P, 4)), ("bcrc", np.uint8, (B, P, 128)), ("hdr", np.int32, (B, P, 9))]
        ptrs = [d.up(np.full(sh, 0x5A, dt)) for _, dt, sh in shapes]
        out = ddn.DmrPduOutput(P, *ptrs)
        rc = d.l.ddn_dmr_pdu_walk_batch(C.byref(inp), self.state, C.byref(out), None)
        assert rc == 0, d.l.ddn_last_error()
        got = {name: d.down(p, dt, sh) for (name, dt, sh), p in zip(shapes, ptrs)}
        for p in d.ptrs[keep:]:
            d.l.ddn_device_free(p)
        del d.ptrs[keep:]
        return got

    def close(self):
        self.d.close()


HDR = ("dpf", "sap", "blocks", "poc", "confirmed", "p_head", "gi", "source", "target")


def check(got, c, outs, pdus, P, nb):
    """channel c of a call against the restatement's outputs of the same bursts"""
    n = len(outs)
    for k, o in enumerate(outs):
        g = (int(got["conf"][c, k]), int(got["counter"][c, k]), int(got["crc"][c, k]), int(got["dbsn"][c, k]), int(got["pick"][c, k]), int(got["status"][c, k]))
        assert g == (o["conf"], o["counter"], o["crc"], o["dbsn"], o["pick"], o["status"]), (c, k, g, o)
    assert not got["status"][c, n:].any() and (got["pick"][c, n:] == -1).all() and (got["dbsn"][c, n:] == 0xFF).all()
    assert int(got["n_pdus"][c]) == len(pdus), (c, int(got["n_pdus"][c]), len(pdus))
    for j, p in enumerate(pdus[:P]):
        assert (int(got["kind"][c, j]), int(got["slot"][c, j]), int(got["burst"][c, j]), int(got["len"][c, j])) == (p["kind"], p["slot"], p["burst"], p["n"]), (c, j)
        assert np.array_equal(got["bytes"][c, j], p["bytes"]), (c, j)
        assert got["crc4"][c, j].tolist() == [p["crc"], p["hdr_crc"], p["blk_crc"], p["pf"]], (c, j, got["crc4"][c, j], p)
        assert np.array_equal(got["bcrc"][c, j, :127], p["valid"]), (c, j)
        assert got["hdr"][c, j].tolist() == [p[k] for k in HDR], (c, j)


_ref = {}


def traffic_of(seed):
    """(FEC-level bursts, marks) of the generated traffic, once per seed"""
    if seed not in _ref:
        items, marks, _ = gen.traffic(seed)
        _ref[seed] = (gen.fec_bursts(items), marks)
    return _ref[seed]


def split_marks(marks, at):
    return [(b, k) for b, k in marks if b < at], [(b - at, k) for b, k in marks if b >= at]


@pytest.mark.parametrize("B", [3, 67])
def test_traffic_in_one_call_and_in_two(built, B):
    """every case of the traffic floors (tests/test_dmr_pdu_traffic.py), each channel its own stream; then the same streams cut in two
    at a different burst per channel - most cuts fall inside a PDU - with the state carried"""
    chans = [traffic_of(c % 3) for c in range(B)]
    P = 8
    w = Walker(B, P)
    nb = max(len(b) for b, _ in chans)
    got = w.call(chans, nb)
    want = {s: dp.walk(*traffic_of(s))[:2] for s in range(3)}
    for c in range(B):
        outs, pdus = want[c % 3]
        assert len(pdus) > P                 # more completed PDUs than slots: the first P stored, all counted
        check(got, c, outs, pdus, P, nb)
    w.close()
    w = Walker(B, P)
    cuts = [5 + (7 * c) % (len(chans[c][0]) - 10) for c in range(B)]
    first = [(chans[c][0][:cuts[c]], split_marks(chans[c][1], cuts[c])[0]) for c in range(B)]
    second = [(chans[c][0][cuts[c]:], split_marks(chans[c][1], cuts[c])[1]) for c in range(B)]
    g1, g2 = w.call(first, nb), w.call(second, nb)
    in_pdu = 0
    for c in range(B):
        st = dp.Walk()
        o1, p1, st = dp.walk(*first[c], state=st)
        p1 = list(p1)
        o2, p2, st = dp.walk(*second[c], state=st)
        check(g1, c, o1, p1, P, nb)
        check(g2, c, o2, p2, P, nb)
        assert [o["status"] for o in o1 + o2] == [o["status"] for o in want[c % 3][0]]
        in_pdu += o2[0]["counter"] > 1 or o2[0]["conf"] == 1
    assert in_pdu >= B // 4
    w.close()


def _conf34(rng, pools):
    """a confirmed rate 3/4 PDU of len(pools) blocks whose pools are made up: each a list of (dbsn, crc ok, metric)"""
    items = [gen.header(0, 3, len(pools))]
    for k, pool in enumerate(pools):
        ents = []
        for dbsn, ok, metric in pool:
            b = gen.block(0, 8, True, rng.integers(0, 256, 16), dbsn=dbsn, good_crc9=bool(ok))["bytes18"]
            ents.append((b, metric, int(ok), dbsn))
        items.append(dict(slot=0, type=8, bytes18=ents[0][0] if ents else np.zeros(18, np.uint8), pool=ents))
    return gen.fec_bursts(items)


def test_pool_pick_tiers(built):
    """dmr_dburst_trellis_choose_candidate_index(): CRC + DBSN, CRC, DBSN, any - the lower metric, the first entry on a tie"""
    rng = np.random.default_rng(5)
    big = [(40 + j, 0, 900 - j) for j in range(30)] + [(7, 1, 50), (2, 1, 60), (2, 1, 55), (2, 1, 55)]       # 34 entries; expected DBSN 2
    pools = [
        [(9, 0, 5), (1, 1, 30), (1, 1, 20), (1, 1, 20)],            # no expectation yet: CRC tier, tie -> index 2, the first of the two
        big,                                                        # CRC + DBSN beats a cheaper CRC-only entry; tie -> index 32
        [(3, 0, 9), (8, 1, 70), (8, 1, 10)],                        # expected 3: no entry has both -> CRC tier (index 2); a sequence error
    ]
    b1 = _conf34(rng, pools)
    pools2 = [
        [(0, 1, 5)],                                                # sets the expectation to 1
        [(4, 0, 1), (1, 0, 9), (1, 0, 7), (1, 0, 7)],               # no CRC anywhere: the DBSN tier, tie -> index 2
        [(4, 0, 3), (5, 0, 2), (6, 0, 2)],                          # nothing matches: the cheapest, tie -> index 1
        [],                                                         # an empty pool: zeros, whose CRC9 checks -> DBSN 0, a sequence error
    ]
    b2 = _conf34(rng, pools2)
    w = Walker(2)
    got = w.call([(b1, []), (b2, [])])
    for c, b in enumerate((b1, b2)):
        outs, pdus, _ = dp.walk(b)
        check(got, c, outs, pdus, 4, max(len(b1), len(b2)))
    assert got["pick"][0, 1:4].tolist() == [2, 32, 2] and got["pick"][1, 1:5].tolist() == [0, 2, 1, -1]
    assert got["status"][0, 3] == dp.ST_SEQ_ERR and got["status"][1, 4] == dp.ST_SEQ_ERR
    w.close()


def test_the_longest_pdu_and_a_counter_that_never_gets_there(built):
    """channel 0: 127 unconfirmed rate 1 blocks, 3048 bytes, CRC32 good.  Channel 1: 127 blocks announced, a header with a bad CRC
    restarts the count after 100 while the byte counter runs on: it saturates at the row's 3072 bytes as
    dmr_block_type1_append_bytes() does, and the PDU that completes there is the row.  Channel 2: an MBC of five continuation blocks
    (refused: more than 4), one of four (the CRC16 window is three blocks: it fails) and one the header of which closes it."""
    rng = np.random.default_rng(6)
    long_items, row = gen.data_pdu(rng, 1, 10, False, 127)
    assert len(row) == 3048
    blocks = [gen.block(0, 10, False, rng.integers(0, 256, 24)) for _ in range(230)]
    sat = [gen.header(0, 2, 127)] + blocks[:100] + [gen.header(0, 2, 3, good_crc=False)] + blocks[100:]
    m5, m4 = gen.mbc(rng, 0, 5), gen.mbc(rng, 1, 4)
    m0 = gen.mbc(rng, 0, 1)[:1]
    m0[0]["bits96"][0] = 1                       # LB in the header itself (its CRC fails with it: header CRC 0)
    chans = [(gen.fec_bursts(x), []) for x in (long_items, sat, m5 + m4 + m0)]
    w = Walker(3)
    got = w.call(chans)
    nb = max(len(b) for b, _ in chans)
    for c, (b, _) in enumerate(chans):
        outs, pdus, st = dp.walk(b)
        check(got, c, outs, pdus, 4, nb)
        if c == 0:
            assert len(pdus) == 1 and pdus[0]["n"] == 3048 and pdus[0]["crc"] == 1 and np.array_equal(pdus[0]["bytes"][:3048], row)
        if c == 1:
            assert len(pdus) == 1 and pdus[0]["n"] == 3072 and pdus[0]["burst"] == 101 + 127
        if c == 2:
            assert [o["status"] for o in outs].count(dp.ST_MBC_LONG) == 1
            assert [(p["n"], p["hdr_crc"], p["blk_crc"]) for p in pdus] == [(60, 1, 0), (24, 0, 0)]
    w.close()


def test_marks_from_events_and_flags(built):
    """ddn_dmr_pdu_marks_batch == dmr_pdu.marks_of on made-up event lists and flag rows, over two calls: the run of quiet symbols is
    carried (1000 at the end of the first call + 800 in the second = a carrier loss at index carry + 799)"""
    d = Dev()
    l = d.l
    B, E, T, stride, nbm, M = 3, 80, 256, 256 + 5000, 6, 16
    state = d.up(np.zeros(B * l.ddn_dmr_pdu_state_bytes(), np.uint8))
    rng = np.random.default_rng(7)

    def run(evs, fls, new, starts):
        ev, ne = np.zeros((B, E, 4), np.int32), np.zeros(B, np.int32)
        for c, rows in enumerate(evs):
            ne[c] = len(rows)
            for i, (pos, kind, a, b, cc) in enumerate(rows):
                ev[c, i] = [pos, kind, a, (b & 0xFFFF) | (cc << 16)]
        fl = np.zeros((B, stride), np.uint8)
        ds, dn = np.full((B, nbm), -1, np.int32), np.zeros(B, np.int32)
        for c in range(B):
            fl[c, T:T + new[c]] = fls[c]
            fl[c, :T] = 1                                    # (the carried records are not looked at)
            dn[c] = len(starts[c])
            ds[c, :dn[c]] = starts[c]
        rb, nr, lb, nl = (d.up(np.full(s, -7, np.int32)) for s in ((B, M), (B,), (B, M), (B,)))
        rc = l.ddn_dmr_pdu_marks_batch(d.up(ev), d.up(ne), E, d.up(fl), stride, T, d.up(np.array(new, np.int32)), d.up(ds), d.up(dn), B, nbm,
                                       state, rb, nr, lb, nl, M, None)
        assert rc == 0, l.ddn_last_error()
        return d.down(rb, np.int32, (B, M)), d.down(nr, np.int32, (B,)), d.down(lb, np.int32, (B, M)), d.down(nl, np.int32, (B,))

    ev0 = [(100, 5, 1, 7, 6), (143, 6, 7, 0, 0), (300, 5, 0, -1, -1), (500, 5, 1, 7, 3 | 1 << 8), (700, 5, 1, 7, 7), (743, 6, 7, 0, 1),
           (900, 8, 0, 1, 0), (950, 8, 1, 1, 1), (1000, 5, 0, -2, -1), (1100, 6, 7, 3, 0), (1200, 7, 0, 25, 1)]
    ev1 = [(10 * i, 5, 0, -1, -1) if i % 3 else (10 * i, 6, 7, 0, i & 1) for i in range(70)]       # more than one chunk of 64
    fl = [np.ones(5000, np.uint8), np.zeros(4100, np.uint8), (rng.random(3000) < 0.0005).astype(np.uint8) * 2]
    fl[0][1100:2899] = 0                                      # 1799 quiet symbols: no loss
    fl[0][4000:5000] = 0                                      # the call ends 1000 symbols into a quiet run
    new = [5000, 4100, 3000]
    pos = [[143, 743], [600, 1799, 1800, 3601], []]
    starts = [[T + p - 143 for p in q] for q in pos]
    rb, nr, lb, nl = run([ev0, ev1, []], fl, new, starts)
    held = [0, 0, 0]
    for c, evs in enumerate([ev0, ev1, []]):
        m = dp.marks_of(evs, fl[c], pos[c])
        r, lo = [b for b, k in m if k == 0], [b for b, k in m if k == 1]
        assert nr[c] == min(len(r), M) and rb[c, :nr[c]].tolist() == r[:M], (c, rb[c], r)
        assert nl[c] == len(lo) and lb[c, :nl[c]].tolist() == lo, (c, lb[c], lo)
        quiet = np.flatnonzero(fl[c] & 3)
        held[c] = len(fl[c]) - (int(quiet[-1]) + 1 if len(quiet) else 0)
    assert nl.tolist()[:2] == [0, 2] and nr[1] == M
    # second call: channel 0 brings 1000 quiet symbols along, 800 more make the loss
    fl2 = [np.zeros(900, np.uint8), np.ones(900, np.uint8), np.zeros(900, np.uint8)]
    fl2[0][850] = 1
    rb, nr, lb, nl = run([[], [], []], fl2, [900, 900, 900], [[T + 700 - 143, T + 850 - 143], [], []])
    assert nl[0] == 1 and lb[0, 0] == 1 and nl[1] == 0 and nr.tolist() == [0, 0, 0]
    d.close()


def test_arguments_are_checked(built):
    l = ddn.lib()
    assert l.ddn_dmr_pdu_walk_batch(None, None, None, None) == ddn.DDN_EINVAL and b"ddn_dmr_pdu_walk_batch" in l.ddn_last_error()
    w = Walker(1, P=9)
    with pytest.raises(AssertionError):
        w.call([(gen.fec_bursts([gen.header(0, 2, 1)]), [])])
    assert b"1 .. 8" in l.ddn_last_error()
    w.close()
