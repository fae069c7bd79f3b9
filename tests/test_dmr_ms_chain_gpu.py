"""GPU: DMR MS / direct-mode traffic through the chain object (ddn_fsk4_chain, protocol DMR, handlers = 1, ddn_fsk4_chain_set_dmr_ms): cu8
I/Q of the generated batch (tests/dmrmsgen.air_batch: eight channels, each with its own delay and noise) in one call, in calls of 200,
3 and 1 symbols (samples_per_call = 10 x symbols), each followed by the flush, against the whole-stream restatement
(tests/dmr_ms.chain_reference over the pinned front end and the oracle loop) burst for burst, and - vocoder = 1 - the PCM of every
channel's talk path bit for bit against the CPU vocoder.  A BS-only stream gives the same ddn_fsk4_chain_results with the feature on."""
import ctypes as C

import numpy as np
import pytest

import chain_fsk4_stream as cs
import ddn
import dmr_ms
import dmrmsgen as gen
import mbe

pytestmark = pytest.mark.gpu
I32, U8, U32, F32 = np.int32, np.uint8, np.uint32, np.float32


def run_chain(x, n, vocoder=1):
    """-> (per channel dict(data, voice, lc: bursts with stream positions and the call that listed them), info).  The input is uploaded
    once; after a call only the four counts per channel come back unless a list holds something"""
    l = ddn.lib()
    B, L = x.shape[:2]
    calls = L // n
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=vocoder)
    ch.set_dmr_ms(1)
    p = cs.upload(l, np.ascontiguousarray(x.reshape(B, calls, n, 2).transpose(1, 0, 2, 3)))
    out = [dict(data=[], voice=[], lc=[]) for _ in range(B)]
    base, news = np.zeros(B, np.int64), []
    f = ch.fetch
    m = None
    for k in range(calls + 1):
        if k < calls:
            ch.run(C.c_void_p(p.value + k * B * n * 2))
        else:
            ch.flush()
        r = ch.results()
        m = m or ch.dmr_ms_results()
        b, d, v = m.bursts, m.data, m.voice
        T, S, md, mv, ml = int(r.carry_symbols), int(m.max_syncs), b.max_data, b.max_voice, b.max_lc
        new, nd, nv, nl = f(r.d_new, I32, (B,)), f(b.d_n_data, I32, (B,)), f(b.d_n_voice, I32, (B,)), f(b.d_n_lc, I32, (B,))
        assert (nd <= md).all() and (nv <= mv).all() and (nl <= ml).all()
        if nd.any():
            a = dict(start=f(b.d_data_start, I32, (B, md)), sync=f(b.d_data_sync, I32, (B, md)), pat=f(b.d_data_pat, U8, (B, md)),
                     slot=f(b.d_data_slot, U8, (B, md)), status=f(b.d_data_status, U8, (B, md)), cc=f(b.d_data_cc, U8, (B, md)),
                     type=f(d.d_type, U8, (B, md)), info=f(d.d_info196, U8, (B, md, 196)), bits96=f(d.d_bits96, U8, (B, md, 96)),
                     bytes12=f(d.d_bytes12, U8, (B, md, 12)), errs=f(d.d_errs, U32, (B, md)), crc=f(d.d_crc, U8, (B, md)),
                     unconfirmed=f(d.d_r34_unconfirmed, U8, (B, md, 18)), confirmed=f(d.d_r34_confirmed, U8, (B, md, 18)),
                     confirmed_crc=f(d.d_r34_confirmed_crc, U8, (B, md)), pool=f(d.d_r34_pool, U8, (B, md, 34, 24)), pool_n=f(d.d_r34_pool_n, I32, (B, md)))
            spos = f(r.d_sync_pos, I32, (B, S))
            for c in range(B):
                for j in range(int(nd[c])):
                    e = {key: val[c, j].copy() for key, val in a.items()}
                    assert e["sync"] // S == c and spos[c, e["sync"] % S] == e["start"] + 89       # the slot it names is its sync
                    e.update(pos=int(base[c]) + int(e["start"]) - T, call=k)
                    out[c]["data"].append(e)
        if nv.any():
            a = dict(start=f(b.d_voice_start, I32, (B, mv)), pre=f(b.d_voice_pre, I32, (B, mv)), vc=f(b.d_voice_vc, U8, (B, mv)),
                     tact_ok=f(b.d_voice_tact_ok, U8, (B, mv)), emb_ok=f(b.d_voice_emb_ok, U8, (B, mv)), emb_cc=f(b.d_voice_emb_cc, U8, (B, mv)),
                     power=f(b.d_voice_power, U8, (B, mv)), sync48=f(b.d_voice_sync48, U8, (B, mv, 48)), frames=f(v.d_ambe_frames, U8, (B, mv, 3, 4, 24)),
                     skip=f(v.d_skip, U8, (B, mv, 3)))
            if vocoder:
                a.update(bits=f(v.d_ambe_bits, U8, (B, mv, 3, 49)), res=f(v.d_ambe_result, I32, (B, mv, 3, 5)), pcm=f(v.d_pcm, F32, (B, mv, 3, 160)))
            for c in range(B):
                assert not a["skip"][c, :nv[c]].any() and (a["skip"][c, nv[c]:] == 0xFF).all()
                assert not vocoder or not a["pcm"][c, nv[c]:].any()
                for j in range(int(nv[c])):
                    e = {key: val[c, j].copy() for key, val in a.items()}
                    e.update(pos=int(base[c]) + int(e["start"]) - T, call=k)
                    out[c]["voice"].append(e)
        if nl.any():
            a = dict(at=f(b.d_lc_pos, I32, (B, ml)), in128=f(b.d_lc_in128, U8, (B, ml, 128)), lc77=f(v.d_lc77, U8, (B, ml, 77)),
                     errs=f(v.d_lc_errs, U32, (B, ml)), ok=f(v.d_lc_ok, U8, (B, ml)))
            for c in range(B):
                for j in range(int(nl[c])):
                    e = {key: val[c, j].copy() for key, val in a.items()}
                    e.update(pos=int(base[c]) + int(e["at"]) - T, call=k)
                    out[c]["lc"].append(e)
        base += new
        news.append(new)
    info = dict(new=np.stack(news), T=T, cc=f(b.d_cc, I32, (B,)), dropped=f(b.d_dropped, I32, (B,)), phase=f(b.d_phase, I32, (B,)),
                dropped_syncs=f(r.d_dropped_syncs, I32, (B,)), vocoder_pointers=(v.d_ambe_bits, v.d_ambe_result, v.d_pcm))
    l.ddn_device_free(p)
    ch.close()
    return out, info


def check_channel(got, ref, ends, T, c, vocoder):
    last = len(ends) - 1
    call_of = lambda p: min(int(np.searchsorted(ends, p, side="right")), last)       # the first call after which record p is held
    assert [e["pos"] for e in got["data"]] == [b["start"] for b in ref["data"]], (c, len(got["data"]), len(ref["data"]))
    for e, b in zip(got["data"], ref["data"]):
        where = (c, b["start"])
        assert (int(e["pat"]), int(e["slot"]), int(e["status"]), int(e["cc"])) == (b["pat"], b["slot"], b["status"], b["cc"]), where
        assert e["call"] == call_of(b["start"] + 89 + T), where                       # the call that holds the carry behind its sync
        if b["status"]:
            assert e["type"] == 0xFF and not e["info"].any() and e["crc"] == 0 and e["pool_n"] == 0, where
            continue
        x = b["fec"]
        assert e["type"] == x["type"] and np.array_equal(e["info"], x["info"]) and e["errs"] == x["errs"] and e["crc"] == x["crc"], where
        if not x["undefined"]:
            assert np.array_equal(e["bits96"], x["bits96"]) and np.array_equal(e["bytes12"], x["bytes12"]), where
        if x["type"] == 8:
            assert np.array_equal(e["unconfirmed"], x["unconfirmed"]) and np.array_equal(e["confirmed"], x["confirmed"]), where
            assert e["confirmed_crc"] == x["confirmed_crc"] and e["pool_n"] == len(x["pool"]), where
            for q, (b18, metric, ok9, dbsn) in zip(e["pool"], x["pool"]):
                assert int(q[:4].copy().view(I32)[0]) == metric and np.array_equal(q[4:22], b18) and (q[22], q[23]) == (ok9, dbsn), where
        else:
            assert e["pool_n"] == 0, where
    assert [e["pos"] for e in got["voice"]] == [v["start"] for v in ref["voice"]], (c, len(got["voice"]), len(ref["voice"]))
    for e, v in zip(got["voice"], ref["voice"]):
        where = (c, v["start"])
        assert [int(e[k]) for k in ("vc", "tact_ok", "emb_ok", "emb_cc", "power")] == [v[k] for k in ("vc", "tact_ok", "emb_ok", "emb_cc", "power")], where
        assert (e["pre"] >= 0) == (v["vc"] == 1) and np.array_equal(e["sync48"], v["sync48"]) and np.array_equal(e["frames"], v["frames"]), where
        assert e["call"] == (call_of(v["start"] + 89 + T) if v["vc"] == 1 else call_of(v["start"] + 143)), where
    assert [e["pos"] for e in got["lc"]] == [x["pos"] for x in ref["lc"]], c
    for e, x in zip(got["lc"], ref["lc"]):
        assert np.array_equal(e["in128"], x["in128"]) and e["errs"] == x["errs"], (c, x["pos"])
        assert x["undefined"] or (np.array_equal(e["lc77"], x["lc77"]) and e["ok"] == x["ok"]), (c, x["pos"])
        assert e["call"] == call_of(x["pos"])
    if vocoder and ref["voice"]:
        frames = np.concatenate([v["frames"] for v in ref["voice"]])
        bits, res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
        pcm, ro = cs.synth_path(ddn.MBE_AMBE, c, bits, res)
        assert np.array_equal(np.concatenate([e["bits"] for e in got["voice"]]), bits), c
        cs._same_pcm(np.concatenate([e["pcm"] for e in got["voice"]]), pcm, c)
        assert np.array_equal(np.concatenate([e["res"] for e in got["voice"]]), ro), c


@pytest.mark.parametrize("symbols", ["one call", 200, 3, 1])
def test_ms_traffic_through_the_chain_object(built, symbols):
    x = gen.air_batch()
    B, L = x.shape[:2]
    n = L if symbols == "one call" else 10 * symbols
    got, info = run_chain(x, n, vocoder=1)
    assert not info["dropped"].any() and not info["dropped_syncs"].any() and not info["new"][-1].any()
    ends = np.cumsum(info["new"], axis=0)
    seen = 0
    for c in range(B):
        ref = dmr_ms.chain_reference(x, c, n)
        assert np.array_equal(ends[:-1, c], ref["held"]), c
        check_channel(got[c], ref, ends[:, c], info["T"], c, 1)
        assert info["cc"][c] == ref["cc"] and info["phase"][c] == 5, c
        seen += len(ref["voice"]) + len(ref["data"])
    assert seen >= 8 * 30


def test_without_a_vocoder_the_voice_pointers_are_null(built):
    x = np.ascontiguousarray(gen.air_batch()[:2, :48000])
    got, info = run_chain(x, 24000, vocoder=0)
    assert info["vocoder_pointers"] == (None, None, None)
    for c in range(2):
        ref = dmr_ms.chain_reference(x, c, 24000, key="short")
        check_channel(got[c], ref, np.cumsum(info["new"], axis=0)[:, c], info["T"], c, 0)
        assert len(ref["voice"]) >= 6


def _main_arrays(r, B, vocoder):
    """every array of ddn_fsk4_chain_results a DMR chain fills: name -> (dtype, shape)"""
    S, st, E, db, lb, vb = int(r.max_syncs), int(r.stride_symbols), r.max_events, r.dmr_data_bursts, r.dmr_emb_lcs, r.dmr_voice_bursts
    a = dict(d_records10=(U8, (B, st, 10)), d_flags=(U8, (B, st)), d_payload2=(U8, (B, st, 2)), d_new=(I32, (B,)), d_counts=(I32, (B,)),
             d_n_sync=(I32, (B,)), d_dropped_syncs=(I32, (B,)), d_sync_pos=(I32, (B, S)), d_sync_pat=(U8, (B, S)), d_pre=(U8, (B, S, 90)),
             d_valid=(U8, (B, S)), d_dmr_slot_type=(U8, (B, S, 20)), d_dmr_slot_type_ok=(U8, (B, S)), d_dmr_pdu96=(U8, (B, S, 96)),
             d_dmr_bptc_errs=(U32, (B, S)), d_events=(I32, (B, E, 4)), d_n_events=(I32, (B,)), d_dmr_n_data=(I32, (B,)),
             d_dmr_data_start=(I32, (B, db)), d_dmr_data_slot=(U8, (B, db)), d_dmr_data_type=(U8, (B, db)), d_dmr_data_info196=(U8, (B, db, 196)),
             d_dmr_data_bits96=(U8, (B, db, 96)), d_dmr_data_bytes12=(U8, (B, db, 12)), d_dmr_data_errs=(U32, (B, db)), d_dmr_data_crc=(U8, (B, db)),
             d_dmr_r34_unconfirmed=(U8, (B, db, 18)), d_dmr_r34_confirmed=(U8, (B, db, 18)), d_dmr_r34_confirmed_crc=(U8, (B, db)),
             d_dmr_r34_pool_n=(I32, (B, db)), d_dmr_n_emb=(I32, (2 * B,)), d_dmr_emb_pos=(I32, (2 * B, lb)), d_dmr_emb_lc77=(U8, (2 * B, lb, 77)),
             d_dmr_emb_errs=(U32, (2 * B, lb)), d_dmr_emb_ok=(U8, (2 * B, lb)))
    if vocoder:
        a.update(d_dmr_n_voice=(I32, (2 * B,)), d_dmr_voice_start=(I32, (2 * B, vb)), d_dmr_voice_pre=(I32, (2 * B, vb)), d_dmr_voice_skip=(U8, (2 * B, vb, 3)),
                 d_dmr_ambe_frames=(U8, (2 * B, vb, 3, 96)), d_dmr_ambe_bits=(U8, (2 * B, vb * 3, 49)), d_dmr_ambe_result=(I32, (2 * B, vb * 3, 5)),
                 d_dmr_pcm=(F32, (2 * B, vb * 3, 160)))
    return a


def _bs_run(x, n, on):
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=1)
    if on:
        ch.set_dmr_ms(1)
    out = []

    def take():
        r = ch.results()
        row = {k: ch.fetch(getattr(r, k), dt, sh) for k, (dt, sh) in _main_arrays(r, B, 1).items()}
        pool_n = row["d_dmr_r34_pool_n"]
        pool = ch.fetch(r.d_dmr_r34_pool, U8, (B, r.dmr_data_bursts, 34, 24))
        row["pool"] = np.concatenate([pool[c, j, :pool_n[c, j]].reshape(-1) for c in range(B) for j in range(r.dmr_data_bursts)] + [np.zeros(0, U8)])
        row["scalars"] = np.array([r.stride_symbols, r.carry_symbols, r.max_syncs, r.voice_slots, r.dmr_voice_bursts, r.max_events, r.dmr_data_bursts,
                                   r.dmr_emb_lcs], np.int64)
        if on:
            m = ch.dmr_ms_results()
            row["ms"] = sum(int(ch.fetch(p, I32, (B,)).sum()) for p in (m.bursts.d_n_data, m.bursts.d_n_voice, m.bursts.d_n_lc))
        out.append(row)

    cs.drive(ch, x, n, take)
    ch.close()
    return out


def test_bs_traffic_is_untouched_and_off_is_the_default(built):
    """a BS-only stream (data bursts of every kind, voice superframes with embedded link control) with the feature on and off: every array
    and count of ddn_fsk4_chain_results is the same bytes call by call, and the MS lists stay empty; off, the getter fails"""
    l = ddn.lib()
    x = np.ascontiguousarray(cs.stream("dmr", "handlers")[:2, :72000])
    off, on = _bs_run(x, 12000, False), _bs_run(x, 12000, True)
    assert len(off) == len(on) == 7
    for a, b in zip(off, on):
        assert b.pop("ms") == 0
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert sum(int(a["d_dmr_n_data"].sum()) for a in off) >= 20 and sum(int(a["d_dmr_n_voice"].sum()) for a in off) >= 6
    ch = ddn.Fsk4ChainC(1, 4800, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=0)
    assert l.ddn_fsk4_chain_get_dmr_ms_results(ch.h, C.byref(ddn.DmrMsChainResults())) == ddn.DDN_EINVAL
    assert b"ddn_fsk4_chain_set_dmr_ms" in l.ddn_last_error()
    for bad in (2, -1):
        assert l.ddn_fsk4_chain_set_dmr_ms(ch.h, bad) == ddn.DDN_EINVAL
    for good in (1, 0):
        assert l.ddn_fsk4_chain_set_dmr_ms(ch.h, good) == 0
    assert l.ddn_fsk4_chain_get_dmr_ms_results(ch.h, C.byref(ddn.DmrMsChainResults())) == ddn.DDN_EINVAL      # switched off again
    assert l.ddn_fsk4_chain_set_dmr_ms(ch.h, 1) == 0 and ch.dmr_ms_results().max_syncs == ch.results().max_syncs
    p = cs.upload(l, np.full((1, 4800, 2), 127, np.uint8))
    ch.run(p)
    assert l.ddn_fsk4_chain_set_dmr_ms(ch.h, 0) == ddn.DDN_EINVAL and b"before its first run" in l.ddn_last_error()        # it has run
    l.ddn_device_free(p)
    ch.close()
    for proto, handlers, inverted in ((ddn.FSK4_DMR, 0, 0), (ddn.FSK4_DMR, 0, 1), (ddn.FSK4_NXDN96, 1, 0)):
        ch = ddn.Fsk4ChainC(1, 4800, proto, rf_mod=2, inverted=inverted, handlers=handlers, vocoder=0)
        assert l.ddn_fsk4_chain_set_dmr_ms(ch.h, 1) == ddn.DDN_EINVAL
        assert l.ddn_fsk4_chain_get_dmr_ms_results(ch.h, C.byref(ddn.DmrMsChainResults())) == ddn.DDN_EINVAL
        ch.close()
