"""GPU: DMR data PDUs through the chain object (ddn_fsk4_chain, protocol DMR, handlers = 1, ddn_fsk4_chain_set_dmr_pdu_slots): cu8 I/Q
of the generated PDU stream (tests/dmrpdugen.air_batch: three channels, one delayed, one starting later) in one call, in three calls
and in calls of 2000 samples (200 symbols: shorter than the 256-symbol carry), each followed by the flush, against the whole-stream
restatement (tests/dmr_pdu.stream_reference over the oracle loop's events and flags) burst for burst and PDU for PDU."""
import ctypes as C

import numpy as np
import pytest

import chain_fsk4_stream as cs
import ddn
import dmr_pdu as dp
import dmrpdugen as gen

pytestmark = pytest.mark.gpu

HDR = ("dpf", "sap", "blocks", "poc", "confirmed", "p_head", "gi", "source", "target")
# the arrays of ddn_fsk4_chain_results a DMR chain with handlers fills: name -> (dtype, shape key)
MAIN = dict(d_n_sync=(np.int32, "B"), d_sync_pos=(np.int32, "BS"), d_sync_pat=(np.uint8, "BS"), d_valid=(np.uint8, "BS"),
            d_dmr_slot_type=(np.uint8, "BS20"), d_dmr_pdu96=(np.uint8, "BS96"), d_dmr_bptc_errs=(np.uint32, "BS"), d_n_events=(np.int32, "B"),
            d_dmr_n_data=(np.int32, "B"), d_dmr_data_start=(np.int32, "BD"), d_dmr_data_slot=(np.uint8, "BD"), d_dmr_data_type=(np.uint8, "BD"),
            d_dmr_data_bytes12=(np.uint8, "BD12"), d_dmr_data_info196=(np.uint8, "BD196"), d_dmr_data_errs=(np.uint32, "BD"),
            d_dmr_data_crc=(np.uint8, "BD"), d_dmr_r34_unconfirmed=(np.uint8, "BD18"), d_dmr_r34_confirmed=(np.uint8, "BD18"),
            d_dmr_r34_pool_n=(np.int32, "BD"), d_dmr_n_emb=(np.int32, "B2"), d_new=(np.int32, "B"), d_counts=(np.int32, "B"))


def _run_chain(x, n, slots=4, main=None):
    """-> (bursts [B]: (absolute position of the last symbol, call, the walk's outputs), pdus [B]: (call, index of the completing burst
    in the channel's stream, fields) of the PDUs stored, info with total [B] = d_n_pdus summed); slots = None leaves the feature off;
    main (a list) receives every call's MAIN arrays"""
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=0)
    if slots:
        ch.set_dmr_pdu_slots(slots)
    bursts, pdus = [[] for _ in range(B)], [[] for _ in range(B)]
    base, total = np.zeros(B, np.int64), np.zeros(B, np.int64)
    calls = [0]

    def take():
        r, f = ch.results(), ch.fetch
        S, T, db = int(r.max_syncs), int(r.carry_symbols), int(r.dmr_data_bursts)
        if main is not None:
            dims = dict(B=(B,), BS=(B, S), BS20=(B, S, 20), BS96=(B, S, 96), BD=(B, db), BD12=(B, db, 12), BD196=(B, db, 196), BD18=(B, db, 18), B2=(2 * B,))
            main.append({k: f(getattr(r, k), dt, dims[sh]) for k, (dt, sh) in MAIN.items()})
        new = f(r.d_new, np.int32, (B,))
        if slots:
            d = ch.dmr_pdu_results()
            o, P = d.out, int(d.out.max_pdus)
            assert int(d.dmr_data_bursts) == db and P == slots
            nd, start = f(r.d_dmr_n_data, np.int32, (B,)), f(r.d_dmr_data_start, np.int32, (B, db))
            per = dict(conf=f(o.d_burst_conf, np.uint8, (B, db)), counter=f(o.d_burst_counter, np.int32, (B, db)), crc=f(o.d_burst_crc, np.uint8, (B, db)),
                       dbsn=f(o.d_burst_dbsn, np.uint8, (B, db)), pick=f(o.d_burst_pick, np.int32, (B, db)), status=f(o.d_burst_status, np.uint8, (B, db)))
            npd = f(o.d_n_pdus, np.int32, (B,))
            pk, ps, pb, pl = f(o.d_pdu_kind, np.uint8, (B, P)), f(o.d_pdu_slot, np.uint8, (B, P)), f(o.d_pdu_burst, np.int32, (B, P)), f(o.d_pdu_len, np.int32, (B, P))
            by, c4 = f(o.d_pdu_bytes, np.uint8, (B, P, 3072)), f(o.d_pdu_crc4, np.uint8, (B, P, 4))
            bc, hd = f(o.d_pdu_block_crc, np.uint8, (B, P, 128)), f(o.d_pdu_header9, np.int32, (B, P, 9))
            for c in range(B):
                total[c] += int(npd[c])
                for j in range(min(int(npd[c]), P)):
                    pdus[c].append((calls[0], len(bursts[c]) + int(pb[c, j]),
                                    dict(kind=int(pk[c, j]), slot=int(ps[c, j]), n=int(pl[c, j]), bytes=by[c, j].copy(), crc4=c4[c, j].tolist(),
                                         valid=bc[c, j, :127].copy(), hdr=hd[c, j].tolist())))
                for k in range(int(nd[c])):
                    bursts[c].append((int(base[c]) + int(start[c, k]) - T + 143, calls[0], {key: int(v[c, k]) for key, v in per.items()}))
        base[:] += new
        calls[0] += 1

    info = {}
    cs.drive(ch, x, n, take, info)
    ch.close()
    cs.check_info(info)
    info["total"] = total
    return bursts, pdus, info


_w = {}


def _want(xc, n):
    import rx4
    key = (xc.ctypes.data, n)
    if key not in _w:
        o = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, rf_mod=2, handler=1))
        w = o.run(cs.front_end_disc(xc, n, 2), max_sync=4096)
        _w[key] = dp.stream_reference(w, o.events.rows())
    return _w[key]


@pytest.mark.parametrize("n", ["one", "three", 2000])
def test_pdu_stream_through_the_chain_object(built, n):
    x = gen.air_batch()
    L = x.shape[1]
    n = {"one": L, "three": L // 3}.get(n, n)
    assert L % n == 0
    P = 8
    bursts, pdus, info = _run_chain(x, n, slots=P)
    across = 0
    for c in range(x.shape[0]):
        pos, fec, marks, outs, want = _want(x[c], n)
        assert [p for p, _, _ in bursts[c]] == pos, (c, len(bursts[c]), len(pos))
        for k, ((p, call, g), o) in enumerate(zip(bursts[c], outs)):
            assert g == {key: o[key] for key in g}, (c, k, g, o)
        ends = np.cumsum(info["new"][:, c])                # symbols of the stream the chain held after each call
        assert int(info["total"][c]) == len(want) >= 9, (c, info["total"][c], len(want))
        stored, seen = [], {}
        for p in want:                                      # a call stores its first P PDUs and counts the rest
            cl = int(np.searchsorted(ends, pos[p["burst"]] + 1, side="left"))
            seen[cl] = seen.get(cl, 0) + 1
            if seen[cl] <= P:
                stored.append(p)
        assert len(pdus[c]) == len(stored) >= 8, (c, len(pdus[c]), len(stored))
        for (call, k, g), p in zip(pdus[c], stored):
            assert (k, g["kind"], g["slot"], g["n"]) == (p["burst"], p["kind"], p["slot"], p["n"]), (c, k, p["burst"])
            assert np.array_equal(g["bytes"], p["bytes"]) and np.array_equal(g["valid"], p["valid"]), (c, k)
            assert g["crc4"] == [p["crc"], p["hdr_crc"], p["blk_crc"], p["pf"]] and g["hdr"] == [p[key] for key in HDR], (c, k)
            # completed once, in the call that holds the last symbol of its last burst
            assert call == bursts[c][k][1] == int(np.searchsorted(ends, pos[k] + 1, side="left")), (c, k, call)
            first = max(j for j in range(k) if fec[j]["type"] in (4, 6) and fec[j]["slot"] == p["slot"])
            across += bursts[c][first][1] < call
    # PDUs whose header lies in an earlier call than their last block.  Every PDU of the stream has two blocks or more, so its header
    # ends 288 symbols or more before its last block does: a call of 2000 samples (about 200 symbols) never holds both.  With three
    # calls only the two boundaries of each channel can fall inside a PDU; the stream puts at least one of them there.
    if n == 2000:
        assert across == sum(len(q) for q in pdus)
    elif n != L:
        assert across >= 1


def test_off_by_default_and_the_main_results_do_not_change(built):
    """without the setter the getter is DDN_EINVAL and nothing is launched; with it, the arrays of ddn_fsk4_chain_results are the same
    bytes call by call; the setter knows its chain"""
    l = ddn.lib()
    x = gen.air_batch()[:, :36000]
    n = 12000
    off, on = [], []
    _run_chain(x, n, slots=None, main=off)
    _run_chain(x, n, slots=2, main=on)
    assert len(off) == len(on) == 4
    for a, b in zip(off, on):
        for k in MAIN:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert sum(int(a["d_dmr_n_data"].sum()) for a in off) > 30
    ch = ddn.Fsk4ChainC(1, 4800, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=0)
    assert l.ddn_fsk4_chain_get_dmr_pdu_results(ch.h, C.byref(ddn.DmrPduChainResults())) == ddn.DDN_EINVAL
    assert b"ddn_fsk4_chain_set_dmr_pdu_slots" in l.ddn_last_error()
    for bad in (0, -1, 9, 1 << 20):
        assert l.ddn_fsk4_chain_set_dmr_pdu_slots(ch.h, bad) == ddn.DDN_EINVAL and b"1 .. 8" in l.ddn_last_error()
    for good in (1, 8, 3):
        assert l.ddn_fsk4_chain_set_dmr_pdu_slots(ch.h, good) == 0
    assert ch.dmr_pdu_results().out.max_pdus == 3
    p = cs.upload(l, np.full((1, 4800, 2), 127, np.uint8))
    ch.run(p)
    assert l.ddn_fsk4_chain_set_dmr_pdu_slots(ch.h, 4) == ddn.DDN_EINVAL                       # it has run
    l.ddn_device_free(p)
    ch.close()
    for proto, handlers in ((ddn.FSK4_DMR, 0), (ddn.FSK4_NXDN48, 1)):
        ch = ddn.Fsk4ChainC(1, 4800, proto, rf_mod=2 if proto == ddn.FSK4_DMR else 0, handlers=handlers, vocoder=0)
        assert l.ddn_fsk4_chain_set_dmr_pdu_slots(ch.h, 4) == ddn.DDN_EINVAL
        assert l.ddn_fsk4_chain_get_dmr_pdu_results(ch.h, C.byref(ddn.DmrPduChainResults())) == ddn.DDN_EINVAL
        ch.close()
