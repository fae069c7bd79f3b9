"""GPU: ddn_dmr_ms_walk_batch / _data_batch / _voice_batch called directly on records built from generator dibits (tests/dmrmsgen.py, no
front end, no receive loop) against the CPU restatement (tests/dmr_ms.py), array for array, call by call.  Every channel carries the
same traffic behind a different number of leading dibits, so the channels of a batch are out of step; the calls are cut so that one
burst of channel 0 ends on a call's last record and another on the next call's first.  Everything but the PCM is integers; the PCM is
compared bit for bit with the CPU vocoder over the talk path's frames."""
import ctypes as C

import numpy as np
import pytest

import chain_fsk4_stream as cs
import ddn
import dmr_ms
import dmrmsgen as gen
import mbe

pytestmark = pytest.mark.gpu

T = 256
GUARD = 64
I32, U8, U32, F32 = np.int32, np.uint8, np.uint32, np.float32
# name -> (dtype, entries per list entry, which list: d data, v voice, l link control, c channel)
BURSTS = dict(d_n_data=(I32, (), "c"), d_data_start=(I32, (), "d"), d_data_sync=(I32, (), "d"), d_data_gate=(I32, (), "d"), d_data_pat=(U8, (), "d"),
              d_data_slot=(U8, (), "d"), d_data_status=(U8, (), "d"), d_data_cc=(U8, (), "d"), d_n_voice=(I32, (), "c"), d_voice_start=(I32, (), "v"),
              d_voice_pre=(I32, (), "v"), d_voice_vc=(U8, (), "v"), d_voice_tact_ok=(U8, (), "v"), d_voice_emb_ok=(U8, (), "v"),
              d_voice_emb_cc=(U8, (), "v"), d_voice_power=(U8, (), "v"), d_voice_sync48=(U8, (48,), "v"), d_n_lc=(I32, (), "c"),
              d_lc_pos=(I32, (), "l"), d_lc_in128=(U8, (128,), "l"), d_cc=(I32, (), "c"), d_dropped=(I32, (), "c"), d_phase=(I32, (), "c"))
DATA = dict(d_type=(U8, (), "d"), d_info196=(U8, (196,), "d"), d_bits96=(U8, (96,), "d"), d_bytes12=(U8, (12,), "d"), d_errs=(U32, (), "d"),
            d_crc=(U8, (), "d"), d_r34_unconfirmed=(U8, (18,), "d"), d_r34_confirmed=(U8, (18,), "d"), d_r34_confirmed_crc=(U8, (), "d"),
            d_r34_pool=(U8, (34, 24), "d"), d_r34_pool_n=(I32, (), "d"))
VOICE = dict(d_ambe_frames=(U8, (3, 4, 24), "v"), d_skip=(U8, (3,), "v"), d_lc77=(U8, (77,), "l"), d_lc_errs=(U32, (), "l"), d_lc_ok=(U8, (), "l"),
             d_ambe_bits=(U8, (3, 49), "v"), d_ambe_result=(I32, (3, 5), "v"), d_pcm=(F32, (3, 160), "v"))


class Dev:
    """device buffers with GUARD marker bytes behind each, checked and freed together"""

    def __init__(self):
        self.l, self.p = ddn.lib(), []

    def up(self, a):
        raw = np.concatenate([np.ascontiguousarray(a).view(U8).reshape(-1), np.full(GUARD, 0xA5, U8)])
        p = C.c_void_p()
        assert self.l.ddn_device_alloc(raw.nbytes, C.byref(p)) == 0 and self.l.ddn_device_upload(p, raw.ctypes.data, raw.nbytes) == 0
        self.p.append((p, a.nbytes))
        return p

    def down(self, p, like):
        a = np.empty_like(like)
        assert self.l.ddn_device_download(a.ctypes.data, p, a.nbytes) == 0
        return a

    def free(self):
        for p, n in self.p:
            g = np.zeros(n + GUARD, U8)
            assert self.l.ddn_device_download(g.ctypes.data, p, g.nbytes) == 0
            assert (g[n:] == 0xA5).all(), "written past the end of an array"
            self.l.ddn_device_free(p)
        self.p = []


def channels(B, seed=5):
    """B channels of the small traffic, channel c behind (53 c) % 288 dibits of its own; the cuts put burst k = 1 of channel 0's unit on
    a call's last record and burst k = 3 on the next call's first -> per channel the calls (tests/dmrmsgen.calls_of)"""
    dib, _ = gen.small_traffic(seed)
    out, ends = [], None
    for c in range(B):
        rng = np.random.default_rng(100 + c)
        mine = np.concatenate([rng.integers(0, 4, (53 * c) % 288).astype(np.int8), dib])
        rec = gen.records(mine, rng)
        syncs = gen.syncs_of(mine, rng)
        if ends is None:
            p = [s[0] for s in syncs if s[1] in dmr_ms.VOICE_PATS][0]
            ends = [700, p + 199 + 288 + 143 + 1, p + 199 + 3 * 288 + 143, 3000]
        out.append(gen.calls_of(rec, syncs, ends + [len(rec)], T))
    return out


def run(chans, caps, vocoder=False):
    """every call of every channel through the three entry points and through the restatement -> the checks; caps = (max_data, max_voice,
    max_lc)"""
    l = ddn.lib()
    B, md, mv, ml = len(chans), *caps
    n_of = dict(d=md, v=mv, l=ml)
    sdev, dev = Dev(), Dev()
    state = sdev.up(np.zeros(B * l.ddn_dmr_ms_state_bytes(), U8))
    assert l.ddn_dmr_ms_state_init(state, B, None) == 0, l.ddn_last_error()
    h = C.c_void_p()
    if vocoder:
        assert l.ddn_mbe_batch_create(ddn.MBE_AMBE, B, C.byref(h)) == 0
    ref = [dmr_ms.State() for _ in range(B)]
    talk = [dict(fr=[], bits=[], pcm=[], res=[]) for _ in range(B)]
    seen = dict(data=0, voice=0, lc=0, dropped=0, refused=0, r34=0)
    for i in range(len(chans[0])):
        calls = [ch[i] for ch in chans]
        stride = max(len(c["row"]) for c in calls) + 1
        S = max(len(c["syncs"]) for c in calls) + 1
        rec = np.zeros((B, stride, 10), U8)
        pos, pat, ns = np.zeros((B, S), I32), np.zeros((B, S), U8), np.zeros(B, I32)
        pre, prel = np.zeros((B, S, 90), U8), np.zeros((B, S, 90), U8)
        for c, call in enumerate(calls):
            rec[c, :len(call["row"])] = call["row"]
            ns[c] = len(call["syncs"])
            for j, (p, pt, a, b) in enumerate(call["syncs"]):
                pos[c, j], pat[c, j], pre[c, j], prel[c, j] = p, pt, a, b
        inp = ddn.DmrMsInput(B, stride, S, dev.up(rec), dev.up(np.array([c["cnt"] for c in calls], I32)), dev.up(np.array([c["new"] for c in calls], I32)),
                             dev.up(pos), dev.up(pat), dev.up(ns), dev.up(pre), dev.up(prel))
        host = {}
        for tab in (BURSTS, DATA, VOICE):
            for k, (dt, sh, which) in tab.items():
                host[k] = np.full((B,) + (() if which == "c" else (n_of[which],)) + sh, 0x5A, dt) if dt != F32 else np.zeros((B, n_of[which]) + sh, F32)
        ptr = {k: dev.up(v) for k, v in host.items()}
        bursts = ddn.DmrMsBursts(md, mv, ml, *[ptr[k] for k in BURSTS])
        data = ddn.DmrMsData(*[ptr[k] for k in DATA])
        voice = ddn.DmrMsVoice(*[ptr[k] if (vocoder or k not in ("d_ambe_bits", "d_ambe_result", "d_pcm")) else None for k in VOICE])
        assert l.ddn_dmr_ms_walk_batch(C.byref(inp), state, C.byref(bursts), None) == 0, l.ddn_last_error()
        assert l.ddn_dmr_ms_data_batch(C.byref(inp), C.byref(bursts), C.byref(data), None) == 0, l.ddn_last_error()
        assert l.ddn_dmr_ms_voice_batch(C.byref(inp), C.byref(bursts), C.byref(voice), h if vocoder else None, None) == 0, l.ddn_last_error()
        g = {k: dev.down(ptr[k], host[k]) for k in host}
        for c, call in enumerate(calls):
            w = dmr_ms.walk_call(ref[c], call["row"][:, 0], call["row"][:, 1], call["cnt"], call["new"], call["syncs"], md, mv, ml)
            where = (i, c)
            assert (g["d_n_data"][c], g["d_n_voice"][c], g["d_n_lc"][c]) == (len(w["data"]), len(w["voice"]), len(w["lc"])), where
            assert (g["d_cc"][c], g["d_dropped"][c], g["d_phase"][c]) == (ref[c].cc, ref[c].dropped, ref[c].next), where
            for k, b in enumerate(w["data"]):
                dmr_ms.finish_data(b)
                got = [int(g[n][c, k]) for n in ("d_data_start", "d_data_sync", "d_data_gate", "d_data_pat", "d_data_slot", "d_data_status", "d_data_cc")]
                assert got == [b["start"], c * S + b["sync"], 0 if b["status"] == 0 else -1, b["pat"], b["slot"], b["status"], b["cc"]], (where, k)
                if b["status"]:
                    seen["refused"] += 1
                    assert g["d_type"][c, k] == 0xFF and not g["d_info196"][c, k].any() and not g["d_bits96"][c, k].any() and g["d_crc"][c, k] == 0
                    assert g["d_r34_pool_n"][c, k] == 0
                    continue
                x = b["fec"]
                assert g["d_type"][c, k] == x["type"] and np.array_equal(g["d_info196"][c, k], x["info"]), (where, k)
                assert g["d_errs"][c, k] == x["errs"] and g["d_crc"][c, k] == x["crc"], (where, k)
                if not x["undefined"]:
                    assert np.array_equal(g["d_bits96"][c, k], x["bits96"]) and np.array_equal(g["d_bytes12"][c, k], x["bytes12"]), (where, k)
                if x["type"] == 8:
                    seen["r34"] += 1
                    assert np.array_equal(g["d_r34_unconfirmed"][c, k], x["unconfirmed"]) and np.array_equal(g["d_r34_confirmed"][c, k], x["confirmed"])
                    assert g["d_r34_confirmed_crc"][c, k] == x["confirmed_crc"] and g["d_r34_pool_n"][c, k] == len(x["pool"]), (where, k)
                    for e, (b18, metric, ok9, dbsn) in zip(g["d_r34_pool"][c, k], x["pool"]):
                        assert int(e[:4].copy().view(I32)[0]) == metric and np.array_equal(e[4:22], b18) and (e[22], e[23]) == (ok9, dbsn), (where, k)
                else:
                    assert g["d_r34_pool_n"][c, k] == 0
            nd = len(w["data"])
            assert (g["d_data_start"][c, nd:] == dmr_ms.UNUSED).all() and (g["d_data_gate"][c, nd:] == -1).all() and (g["d_type"][c, nd:] == 0xFF).all()
            for k, v in enumerate(w["voice"]):
                got = [int(g[n][c, k]) for n in ("d_voice_start", "d_voice_pre", "d_voice_vc", "d_voice_tact_ok", "d_voice_emb_ok", "d_voice_emb_cc", "d_voice_power")]
                assert got == [v["start"], -1 if v["pre"] < 0 else c * S + v["pre"], v["vc"], v["tact_ok"], v["emb_ok"], v["emb_cc"], v["power"]], (where, k)
                assert np.array_equal(g["d_voice_sync48"][c, k], v["sync48"]) and np.array_equal(g["d_ambe_frames"][c, k], v["frames"]), (where, k)
                assert not g["d_skip"][c, k].any()
                talk[c]["fr"].append(v["frames"])
                if vocoder:
                    talk[c]["bits"].append(g["d_ambe_bits"][c, k])
                    talk[c]["pcm"].append(g["d_pcm"][c, k])
                    talk[c]["res"].append(g["d_ambe_result"][c, k])
            nv = len(w["voice"])
            assert (g["d_voice_start"][c, nv:] == dmr_ms.UNUSED).all() and not g["d_voice_vc"][c, nv:].any() and (g["d_skip"][c, nv:] == 0xFF).all()
            assert not g["d_ambe_frames"][c, nv:].any() and (not vocoder or not g["d_pcm"][c, nv:].any())
            for k, x in enumerate(w["lc"]):
                assert g["d_lc_pos"][c, k] == x["pos"] and np.array_equal(g["d_lc_in128"][c, k], x["in128"]) and g["d_lc_errs"][c, k] == x["errs"], (where, k)
                assert x["undefined"] or (np.array_equal(g["d_lc77"][c, k], x["lc77"]) and g["d_lc_ok"][c, k] == x["ok"]), (where, k)
            assert (g["d_lc_pos"][c, len(w["lc"]):] == -1).all() and not g["d_lc_ok"][c, len(w["lc"]):].any()
            seen["data"] += nd
            seen["voice"] += nv
            seen["lc"] += len(w["lc"])
        dev.free()
    seen["dropped"] = sum(s.dropped for s in ref)
    if vocoder:
        for c in range(B):
            frames = np.concatenate(talk[c]["fr"])
            bits, res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
            pcm, ro = cs.synth_path(ddn.MBE_AMBE, c, bits, res)
            assert np.array_equal(np.concatenate(talk[c]["bits"]), bits), c
            cs._same_pcm(np.concatenate(talk[c]["pcm"]), pcm, c)
            assert np.array_equal(np.concatenate(talk[c]["res"]), ro), c
        l.ddn_mbe_batch_destroy(h)
    sdev.free()
    return seen


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_the_three_calls_equal_the_restatement(built, B):
    seen = run(channels(B), (4, 4, 2), vocoder=B == 1)
    assert seen == dict(data=4 * B, voice=6 * B, lc=B, dropped=0, refused=B, r34=B)


def test_the_cuts_put_a_burst_on_a_call_s_last_and_on_the_next_call_s_first_record(built):
    calls = channels(1)[0]
    ends = np.cumsum([c["new"] for c in calls])
    p = [s[0] + c["lo"] for c in calls for s in c["syncs"] if s[1] in dmr_ms.VOICE_PATS][0]
    assert p + 199 + 288 + 143 == ends[1] - 1 and p + 199 + 3 * 288 + 143 == ends[2]


def test_a_list_one_entry_too_small_drops_and_counts(built):
    """one call holds the whole stream: 4 data bursts, 6 voice bursts, 1 link control.  Lists of 3, 5 and 1: one burst of each kind is
    counted in d_dropped and nothing is written behind the lists' ends (guard bytes behind every array)"""
    dib, _ = gen.small_traffic()
    rng = np.random.default_rng(9)
    rec, syncs = gen.records(dib, rng), gen.syncs_of(dib, rng)
    whole = [dict(row=rec, cnt=len(rec), new=len(rec), syncs=syncs, lo=0)]
    assert run([whole], (4, 6, 1))["dropped"] == 0
    seen = run([whole], (3, 5, 1))
    assert seen["dropped"] == 2 and (seen["data"], seen["voice"], seen["lc"]) == (3, 5, 1)
    whole2 = [dict(row=np.concatenate([rec, rec]), cnt=2 * len(rec), new=2 * len(rec),
                   syncs=syncs + [(p + len(rec), pat, a, b) for p, pat, a, b in syncs], lo=0)]
    assert run([whole2], (8, 12, 1))["dropped"] == 1
