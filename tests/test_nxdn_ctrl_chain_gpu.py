"""GPU: NXDN control and data channels through the chain object (ddn_fsk4_chain, protocol NXDN96 / NXDN48, handlers = 1,
ddn_fsk4_chain_set_nxdn_ctrl): cu8 I/Q of the generated batch (tests/nxdngen.air_batch: three channels - as sent, delayed, starting later)
in one call, in three calls and in calls of 200 symbols (shorter than the 256-symbol carry), each followed by the flush, against the
whole-stream restatement (tests/nxdn_ctrl.stream_reference over the oracle loop) frame for frame and message for message."""
import ctypes as C

import numpy as np
import pytest

import chain_fsk4_stream as cs
import ddn
import nxdn_ctrl as nc
import nxdngen as gen
import rx4

pytestmark = pytest.mark.gpu

# the arrays of ddn_fsk4_chain_results an NXDN chain fills: name -> (dtype, trailing shape)
MAIN = dict(d_n_sync=(np.int32, None), d_sync_pos=(np.int32, ()), d_sync_pat=(np.uint8, ()), d_pre=(np.uint8, (90,)), d_valid=(np.uint8, ()),
            d_nxdn_lich=(np.uint8, ()), d_nxdn_sacch=(np.uint8, (4,)), d_nxdn_sacch_ok=(np.uint8, ()), d_nxdn_sacch_hard=(np.uint8, (32,)),
            d_nxdn_sacch_hard_ok=(np.uint8, ()), d_nxdn_facch=(np.uint8, (2, 12)), d_nxdn_facch_ok=(np.uint8, (2,)), d_new=(np.int32, None),
            d_counts=(np.int32, None), d_dropped_syncs=(np.int32, None))


def _run_chain(x, n, which="nxdn96", on=True, main=None):
    """-> (units [B]: (absolute sync position, call, valid, the stage's fields of the slot), info); on = False leaves the feature off;
    main (a list) receives every call's MAIN arrays"""
    B = x.shape[0]
    row = cs.NXDN[which]
    ch = ddn.Fsk4ChainC(B, n, row["gpu"], rf_mod=row["rf_mod"], handlers=1, vocoder=0)
    if on:
        ch.set_nxdn_ctrl(1)
    units = [[] for _ in range(B)]
    base, calls = np.zeros(B, np.int64), [0]

    def take():
        r, f = ch.results(), ch.fetch
        S, T = int(r.max_syncs), int(r.carry_symbols)
        if main is not None:
            main.append({k: f(getattr(r, k), dt, (B,) if sh is None else (B, S) + sh) for k, (dt, sh) in MAIN.items()})
        ns, pos, new = f(r.d_n_sync, np.int32, (B,)), f(r.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,))
        if on:
            cr = ch.nxdn_ctrl_results()
            assert int(cr.max_syncs) == S and cr.d_sync_pos == r.d_sync_pos and cr.d_valid == r.d_valid
            a = {k: f(getattr(cr.frames, "d_" + k), dt, (B, S) + sh) for k, (dt, sh) in nc.FRAME_ARRAYS.items()}
            a.update({k: f(getattr(cr.messages, "d_" + k), dt, (B, S) + sh) for k, (dt, sh) in nc.MESSAGE_ARRAYS.items()})
            valid = f(cr.d_valid, np.uint8, (B, S))
            for c in range(B):
                for k in range(int(ns[c])):
                    units[c].append((int(base[c]) + int(pos[c, k]) - T, calls[0], int(valid[c, k]), {key: v[c, k].copy() for key, v in a.items()}))
        base[:] += new
        calls[0] += 1

    info = {}
    cs.drive(ch, x, n, take, info)
    ch.close()
    cs.check_info(info)
    return units, info


_w = {}


def _want(which, c, n):
    key = (which, c, n)
    if key not in _w:
        x = gen.air_batch(which)
        _w[key] = nc.stream_reference(cs.nxdn_oracle_stream(x[c], n, which))
    return _w[key]


def _check_channel(units, ref, ends, T, where):
    """every whole frame of the reference once, under its position, field for field, in the call that decodes it: the first one that
    holds the T carried records behind its sync (a frame is 182 symbols, T is 256), else the flush; -> the calls (first segment, last
    frame) of every delivered superframe"""
    whole = [u for u in units if u[2]]
    assert len({p for p, _, _, _ in units}) == len(units), "a frame decoded twice"
    assert [p for p, _, _, _ in whole] == [p for p, _, _ in ref], (where, len(whole), len(ref))
    spans, first = [], None
    for (p, call, _, g), (_, fr, w) in zip(whole, ref):
        assert int(g["kind"]) == fr["kind"], (where, p)
        if fr["kind"]:
            for k in ("bits208", "bytes26", "crc_ok", "fallback", "ran", "sf"):
                assert np.array_equal(g[k], fr[k]), (where, p, k)
        for k in ("sacch_status", "pf", "seq_ok", "msg_status", "last_ran", "cac_fail"):
            assert int(g[k]) == int(w[k]), (where, p, k, int(g[k]), w[k])
        if w["msg72"] is not None:
            assert np.array_equal(g["msg72"], w["msg72"]), (where, p)
        # decoded - and its message delivered - once, in that call
        assert call == min(int(np.searchsorted(ends, p + T + 1, side="left")), len(ends) - 1), (where, p, call)
        if w["sacch_status"] == 1 and w["pf"] == 0:
            first = call
        if w["sacch_status"] == 1 and w["msg_status"] == 1:
            spans.append((first, call))
    return spans


@pytest.mark.parametrize("which,n", [("nxdn96", "one"), ("nxdn96", "three"), ("nxdn96", 2000), ("nxdn48", "one"), ("nxdn48", "three"), ("nxdn48", 4000)])
def test_control_stream_through_the_chain_object(built, which, n):
    x = gen.air_batch(which)
    L = x.shape[1]
    short = n in (2000, 4000)
    n = {"one": L, "three": L // 3}.get(n, n)
    assert L % n == 0
    units, info = _run_chain(x, n, which)
    delivered = 0
    for c in range(x.shape[0]):
        ref = _want(which, c, n)
        ends = np.cumsum(info["new"][:, c])                  # symbols of the stream the chain held after each call
        spans = _check_channel(units[c], ref, ends, info["T"], (which, c))
        assert len(spans) == sum(w["msg_status"] == 1 and w["sacch_status"] == 1 for _, _, w in ref) >= 2
        delivered += len(spans)
        if short:
            # four frames of 192 symbols against calls of 200: every delivered superframe crosses three call boundaries or more
            assert all(b - a >= 3 for a, b in spans), spans
        elif n != L:
            assert all(b >= a for a, b in spans)
    assert delivered >= (12 if which == "nxdn96" else 5)


def test_off_by_default_and_the_main_results_do_not_change(built):
    """without the setter the getter is DDN_EINVAL and names the setter; with it, the arrays of ddn_fsk4_chain_results are the same bytes
    call by call; the setter knows its chain"""
    l = ddn.lib()
    x = np.ascontiguousarray(gen.air_batch("nxdn96")[:, :72000])
    n = 24000
    off, on = [], []
    _run_chain(x, n, on=False, main=off)
    _run_chain(x, n, on=True, main=on)
    assert len(off) == len(on) == 4
    for a, b in zip(off, on):
        for k in MAIN:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert sum(int(a["d_n_sync"].sum()) for a in off) > 60
    ch = ddn.Fsk4ChainC(1, 4800, ddn.FSK4_NXDN96, rf_mod=2, handlers=1, vocoder=0)
    assert l.ddn_fsk4_chain_get_nxdn_ctrl_results(ch.h, C.byref(ddn.NxdnCtrlChainResults())) == ddn.DDN_EINVAL
    assert b"ddn_fsk4_chain_set_nxdn_ctrl" in l.ddn_last_error()
    for bad in (2, -1):
        assert l.ddn_fsk4_chain_set_nxdn_ctrl(ch.h, bad) == ddn.DDN_EINVAL
    for good in (1, 0, 1):
        assert l.ddn_fsk4_chain_set_nxdn_ctrl(ch.h, good) == 0
    assert ch.nxdn_ctrl_results().max_syncs == ch.results().max_syncs
    p = cs.upload(l, np.full((1, 4800, 2), 127, np.uint8))
    ch.run(p)
    assert l.ddn_fsk4_chain_set_nxdn_ctrl(ch.h, 1) == ddn.DDN_EINVAL and b"before its first run" in l.ddn_last_error()        # it has run
    l.ddn_device_free(p)
    ch.close()
    for proto, handlers in ((ddn.FSK4_DMR, 1), (ddn.FSK4_NXDN48, 0), (ddn.FSK4_NXDN96, 0)):
        ch = ddn.Fsk4ChainC(1, 4800, proto, rf_mod=2 if proto != ddn.FSK4_NXDN48 else 0, handlers=handlers, vocoder=0)
        assert l.ddn_fsk4_chain_set_nxdn_ctrl(ch.h, 1) == ddn.DDN_EINVAL
        assert l.ddn_fsk4_chain_get_nxdn_ctrl_results(ch.h, C.byref(ddn.NxdnCtrlChainResults())) == ddn.DDN_EINVAL
        ch.close()


def test_nxdn48_capture_delivers_vcall_source_901(built):
    """the reference's NXDN48 capture through the chain with the feature on: the messages the library delivers include the VCALLs with
    source unit 901 under RAN 1 - "Src=901", the string DECODE_IQ_NXDN48 asserts"""
    iq = cs._golden_iq("iq_nxdn48.npz")
    n = 72000
    x = np.ascontiguousarray(iq[None, :len(iq) - len(iq) % n])
    units, info = _run_chain(x, n, "nxdn48")
    msgs = [(int(g["last_ran"]), g["msg72"]) for _, _, v, g in units[0] if v and int(g["msg_status"]) == 1]
    vcall = [m for _, m in msgs if rx4.bits_int(m[2:8]) == 1]
    assert len(vcall) >= 4 and all(rx4.bits_int(m[24:40]) == 901 for m in vcall) and all(ran == 1 for ran, _ in msgs)
    ref = nc.stream_reference(cs.nxdn_oracle_stream(x[0], n, "nxdn48"))
    _check_channel(units[0], ref, np.cumsum(info["new"][:, 0]), info["T"], "capture")
