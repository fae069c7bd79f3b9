"""dPMR (-fm) superframes and voice on the device: ddn_dpmr_superframe_decode_batch / _identity_batch / _voice_gather against the CPU
restatement (tests/dpmr.py) on the oracle loop's records of the reference's capture and on generated superframes; then the fsk4 chain
object with DDN_FSK4_DPMR from cu8 I/Q - "Src=1601621" (DECODE_IQ_DPMR, tests/CMakeLists.txt:8950), the -xd reading, a batch of
delayed / negated / late channels, the voice halves through AMBE 3600x2450 synthesis, and the configuration rules."""
import ctypes as C

import numpy as np
import pytest

import ddn
import dpmr
import dpmrgen
import mbe
import rx4

# the per-slot checks, the chain's collector, its whole-stream reference and its checks live in tests/chain_fsk4_stream.py (the
# short-call tests share them)
from chain_fsk4_stream import DPMR_VOICE_PLAN as VOICE_PLAN
from chain_fsk4_stream import dpmr_aiid as aiid
from chain_fsk4_stream import dpmr_check_chain_channel as check_chain_channel
from chain_fsk4_stream import dpmr_check_chain_voice as check_chain_voice
from chain_fsk4_stream import dpmr_check_identity as check_identity
from chain_fsk4_stream import dpmr_check_superframe as check_superframe
from chain_fsk4_stream import dpmr_check_voice_slot as check_voice_slot
from chain_fsk4_stream import dpmr_oracle_stream as oracle_stream
from chain_fsk4_stream import dpmr_run_chain as run_chain
from chain_fsk4_stream import dpmr_voice_transmission as _voice_transmission

pytestmark = pytest.mark.gpu

N_CALL = 48000


# ---- the batch entries on records built on the host ---------------------------------------------------------------------------------
def device_decode(streams, syncs, inverted, state=None):
    """streams: per channel the record dibits; syncs: per channel the sync positions -> every per-slot output as numpy"""
    import torch
    l = ddn.lib()
    B = len(streams)
    stride = max(len(s) for s in streams) + 8
    M = max(1, max(len(s) for s in syncs))
    rec = np.zeros((B, stride, 10), np.uint8)
    cnt = np.zeros(B, np.int32)
    pos = np.zeros((B, M), np.int32)
    ns = np.zeros(B, np.int32)
    for c in range(B):
        rec[c, :len(streams[c]), 0] = streams[c]
        rec[c, :len(streams[c]), 1] = 200          # (a reliability byte that must not leak into the dibit)
        cnt[c], ns[c] = len(streams[c]), len(syncs[c])
        pos[c, :len(syncs[c])] = syncs[c]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    p = lambda x: x.data_ptr()
    d_rec, d_cnt, d_pos, d_ns = t(rec), t(cnt), t(pos), t(ns)
    o = dict(bits=z((B, M, 2, 48), torch.uint8), ham=z((B, M, 2, 6), torch.uint8), crc=z((B, M, 2), torch.uint8),
             fields=z((B, M, 2, 8), torch.int32), id=z((B, M), torch.int32), color=z((B, M), torch.int32), valid=z((B, M), torch.uint8),
             kind=z((B, M), torch.uint8), strong=z((B, M), torch.uint8), tg=z((B, M), torch.int32), src=z((B, M), torch.int32),
             fr=z((B, M, 8, 4, 24), torch.uint8), voiced=z((B, M, 2), torch.uint8), muted=z((B, M, 2), torch.uint8))
    st = t(np.array([[-1, -1, 0]] * B, np.int32) if state is None else state)
    assert l.ddn_dpmr_superframe_decode_batch(p(d_rec), stride, p(d_cnt), p(d_pos), p(d_ns), B, M, inverted, p(o["bits"]), p(o["ham"]),
                                              p(o["crc"]), p(o["fields"]), p(o["id"]), p(o["color"]), p(o["valid"]), None) == 0
    assert l.ddn_dpmr_identity_batch(p(d_ns), B, M, p(o["valid"]), p(o["fields"]), p(o["ham"]), p(o["crc"]), p(o["id"]), p(st), p(o["kind"]),
                                     p(o["strong"]), p(o["tg"]), p(o["src"]), None) == 0
    assert l.ddn_dpmr_voice_gather(p(d_rec), stride, p(d_pos), p(d_ns), B, M, inverted, p(o["fields"]), p(o["valid"]), p(o["fr"]), p(o["voiced"]),
                                   p(o["muted"]), None) == 0
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["state"] = st.cpu().numpy()
    return out


def test_superframe_kernels_on_the_capture_records_under_both_words(built):
    disc = rx4.capture_disc("iq_dpmr.npz", 1)
    for inverted in (0, 1):
        o = rx4.OracleFsk4Rx(dpmr.profile(inverted)).run(disc)
        dib, sp = o["rec4"][:, 0].astype(np.uint8), np.asarray(o["sync_pos"])
        got = device_decode([dib], [sp], inverted)
        want = dpmr.decode_stream(dib, sp, inverted)
        assert len(want) >= (50 if inverted else 5)     # (the capture is sent inverted: plain -fm locks on a handful of superframes)
        for k, sf in want:
            assert got["valid"][0, k] == 1
            check_superframe(got, 0, k, sf)
            check_identity(got, 0, k, sf)
            check_voice_slot(got, 0, k, sf)
        for k in set(range(len(sp))) - {k for k, _ in want}:
            assert got["valid"][0, k] == 0 and got["color"][0, k] == -1
        if inverted == 0:
            assert got["state"][0, 1] >= 0 and aiid(got["state"][0, 1]) == "1601621"


def _generated(rng, n_sf, inverted):
    """superframes with 0 / 1 / 2 bit errors per Hamming word, bad CRCs, unknown colour codes, every frame-number pair"""
    sfs = []
    for i in range(n_sf):
        cch = []
        for h in range(2):
            fn = [(0, 1), (2, 3), (1, 0), (3, 2), (0, 3)][i % 5][h]
            bits = dpmrgen.cch_bits(fn=fn, half=int(rng.integers(0, 4096)), mode=int(rng.integers(0, 8)), version=int(rng.integers(0, 4)),
                                    format=int(rng.integers(0, 4)), emergency=int(rng.integers(0, 2)), reserved=int(rng.integers(0, 2)),
                                    slow=int(rng.integers(0, 1 << 18)), crc_good=rng.random() > 0.25)
            flips = []
            for j in range(6):
                ne = int(rng.choice([0, 0, 1, 2]))
                flips += [(j, int(b)) for b in rng.choice(12, ne, replace=False)]
            cch.append(dpmrgen.cch_dibits(bits, flips))
        col = dpmrgen.color_pattern(int(rng.integers(0, 64))) if rng.random() > 0.3 else int(rng.integers(0, 1 << 24))
        sfs.append(dpmrgen.superframe(cch[0], cch[1], col, rng.integers(0, 4, (8, 36))))
    d = dpmrgen.transmission(sfs, inverted=bool(inverted))
    return np.concatenate([rng.integers(0, 4, 50).astype(np.uint8), d])


def test_superframe_kernels_on_generated_superframes(built):
    rng = np.random.default_rng(23)
    for inverted in (0, 1):
        streams, syncs = [], []
        for c in range(3):
            d = _generated(rng, 30, inverted)
            cut = len(d) - 100 * c                     # channels 1 / 2: the last superframe is not whole
            streams.append(d[:cut])
            syncs.append([50 + 384 * i + 11 for i in range(30)])
        got = device_decode(streams, syncs, inverted)
        n_bad_ham = n_bad_crc = n_nocol = 0
        for c in range(3):
            want = dpmr.decode_stream(streams[c], syncs[c], inverted)
            assert len(want) == (30 if c == 0 else 29)
            for k, sf in want:
                check_superframe(got, c, k, sf)
                check_identity(got, c, k, sf)
                check_voice_slot(got, c, k, sf)
                n_bad_ham += sum(not h["ham_ok"] for h in sf["cch"])
                n_bad_crc += sum(not h["crc_ok"] for h in sf["cch"])
                n_nocol += sf["color"] < 0
            if c:
                assert got["valid"][c, 29] == 0
        assert n_bad_ham > 10 and n_bad_crc > 10 and n_nocol > 5


# ---- the chain object -------------------------------------------------------------------------------------------------------------
def _upload(l, part):
    p = C.c_void_p()
    assert l.ddn_device_alloc(part.nbytes, C.byref(p)) == 0 and l.ddn_device_upload(p, part.ctypes.data, part.nbytes) == 0
    return p


def _capture_iq():
    from conftest import golden
    return np.ascontiguousarray(golden("iq_dpmr.npz")["iq"], np.uint8)


def _delay(iq, d, rng):
    out = np.empty_like(iq)
    out[:d] = np.clip(np.rint(127.5 + rng.normal(0, 3, (d, 2))), 0, 255).astype(np.uint8)
    out[d:] = iq[:len(iq) - d]
    return out


def test_chain_fm_known_answer_batch_and_voice(built):
    """-fm: five channels (the capture; delayed by 12345 and by 777 samples; negated - I/Q swapped, the other polarity; silent for its
    first 30 000 samples), 48 000-sample calls + flush, vocoder = 1: every channel equals its own oracle stream field for field (identity
    state per channel, carried across calls), the voice equals the CPU vocoder; the capture reads Src=1601621 from the first strong
    calling part on, TG ends at 6038584 (plain -fm locks on a handful of its superframes: the capture is sent inverted); the negated
    channel is the -xd reading (TG = Src = 3939*5*) with a superframe across most seams"""
    iq = _capture_iq()
    rng = np.random.default_rng(4)
    x = np.stack([iq, _delay(iq, 12345, rng), _delay(iq, 777, rng), iq[:, ::-1], iq.copy()])
    x[4, :30000] = 127
    sfs, voice, seams = run_chain(x, N_CALL)
    assert seams >= 5
    total = 0
    for c in range(x.shape[0]):
        want = oracle_stream(x[c], N_CALL)
        got = check_chain_channel(sfs[c], want)
        total += check_chain_voice(voice[c], want, c)
        if c != 3:
            assert len(got) >= 5, (c, len(got))
            srcs = [aiid(g["src"]) for _, g in got]
            first = [i for i, (_, g) in enumerate(got) if g["kind"] == 2 and g["strong"]][0]
            assert srcs[first] == "1601621" and all(s == "1601621" for s in srcs[first:]), (c, srcs)
            assert aiid(got[-1][1]["tg"]) == "6038584", c
        else:
            assert len(got) >= 50 and aiid(got[-1][1]["tg"]) == "3939*5*" and aiid(got[-1][1]["src"]) == "3939*5*"
    assert total >= 400


def test_chain_fm_ragged_calls(built):
    """the capture in 29 989-sample calls (every seam somewhere else inside a superframe), vocoder = 0: as sent, rotated by 5000
    samples, negated"""
    iq = _capture_iq()
    n = 29989
    L = (len(iq) // n) * n
    x = np.stack([iq[:L], np.roll(iq, 5000, axis=0)[:L], iq[:L, ::-1]])
    sfs, _, seams = run_chain(x, n, vocoder=0)
    assert seams >= 5
    for c in range(3):
        got = check_chain_channel(sfs[c], oracle_stream(x[c], n))
        assert len(got) >= (50 if c == 2 else 5)
        if c < 2:
            assert aiid(got[-1][1]["src"]) == "1601621"


def test_chain_xd(built):
    """-xd (inverted = 1): the capture's superframes with both CRCs good, frame numbers (0, 1) / (2, 3), TG = Src = 3939*5*, channel code 2"""
    iq = _capture_iq()
    sfs, voice, seams = run_chain(iq[None], N_CALL, inverted=1)
    assert seams >= 5
    want = oracle_stream(iq, N_CALL, inverted=1)
    got = check_chain_channel(sfs[0], want)
    check_chain_voice(voice[0], want, 0)
    good = [g for _, g in got if g["crc"].all()]
    assert len(good) >= 45
    assert {(int(g["fields"][0, 0]), int(g["fields"][1, 0])) for g in good} == {(0, 1), (2, 3)}
    assert {int(g["color"]) for g in good} == {2}
    assert aiid(got[-1][1]["tg"]) == "3939*5*" and aiid(got[-1][1]["src"]) == "3939*5*"


def test_generated_voice_through_the_batch_entries(built):
    """generated superframes (communication modes 0 / 1 / 5 / other, version 3 in either half) through ddn_dpmr_* on records built on the
    host, the voiced halves' frames through ddn_mbe_frame_decode_batch + ddn_mbe_synth_batch, one talk path per channel: frames, flags,
    PCM and result rows == the restatement + the oracle frame FEC + the CPU vocoder"""
    import torch
    l = ddn.lib()
    rng = np.random.default_rng(17)
    streams, syncs, inv = [], [], 0
    for c in range(2):
        sfs = _voice_transmission(rng, VOICE_PLAN)
        streams.append(np.concatenate([rng.integers(0, 4, 20).astype(np.uint8), dpmrgen.transmission(sfs)]))
        syncs.append([20 + 384 * i + 11 for i in range(len(sfs))])
    got = device_decode(streams, syncs, inv)
    for c in range(2):
        want = dpmr.decode_stream(streams[c], syncs[c], inv)
        assert len(want) == len(VOICE_PLAN)
        fr, mut = [], []
        for k, sf in want:
            check_superframe(got, c, k, sf)
            check_voice_slot(got, c, k, sf)
            for h in range(2):
                if got["voiced"][c, k, h]:
                    fr += list(got["fr"][c, k, 4 * h:4 * h + 4])
                    mut += [int(got["muted"][c, k, h])] * 4
        assert sum(mut) > 0 and len(fr) == 4 * sum(sum(dpmr.voice_halves(sf)) for _, sf in want)
        frames = np.ascontiguousarray(np.stack(fr))
        F = len(frames)
        d_fr = torch.from_numpy(frames).cuda()
        d_bits, d_res = torch.zeros((F, 49), dtype=torch.uint8, device="cuda"), torch.zeros((F, 5), dtype=torch.int32, device="cuda")
        assert l.ddn_mbe_frame_decode_batch(ddn.MBE_AMBE, d_fr.data_ptr(), None, F, d_bits.data_ptr(), d_res.data_ptr(), None) == 0
        h = C.c_void_p()
        assert l.ddn_mbe_batch_create(ddn.MBE_AMBE, 1, C.byref(h)) == 0
        d_pcm, d_ro = torch.zeros((F, 160), dtype=torch.float32, device="cuda"), torch.zeros((F, 5), dtype=torch.int32, device="cuda")
        for a in range(0, F, 8):        # a superframe's worth per call, the talk path's history carried (as the chain's calls do)
            b = min(F, a + 8)
            assert l.ddn_mbe_synth_batch(h, d_bits[a:].data_ptr(), d_res[a:].data_ptr(), b - a, d_pcm[a:].data_ptr(), d_ro[a:].data_ptr(),
                                         None) == 0
        torch.cuda.synchronize()
        l.ddn_mbe_batch_destroy(h)
        bits, res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
        assert np.array_equal(d_bits.cpu().numpy(), bits) and np.array_equal(d_res.cpu().numpy(), res)
        voc = mbe.OracleVocoder(ddn.MBE_AMBE, 1)
        pcm, ro, rc = voc.run(bits[None], res[None])
        assert rc == 0
        gp = d_pcm.cpu().numpy()
        bad = [j for j in range(F) if not np.array_equal(gp[j].view(np.uint32), pcm[0, j].view(np.uint32))]
        assert not bad, (c, F, bad[:8])
        assert np.array_equal(d_ro.cpu().numpy(), ro[0])


def test_generated_voice_through_the_chain(built):
    """the generated transmission as cu8 (p25gen.modulate_cu8 at 20 samples per symbol, 2400 symbols/s) in two channels (the second
    -xd: every dibit ^ 2), 48 000-sample calls + flush: the chain equals the oracle pipeline on the same samples - superframes,
    identity, the voiced halves in air order with their muted flags, PCM and result rows"""
    import p25gen
    rng = np.random.default_rng(29)
    sfs = _voice_transmission(rng, VOICE_PLAN)
    n = 5 * N_CALL
    out = []
    for inverted in (0, 1):
        dib = dpmrgen.transmission(sfs, inverted=bool(inverted))
        x = p25gen.modulate_cu8(dib, n, sps=20, dev=0.045, lead=1000 + 333 * inverted, seed=inverted)
        got_sfs, voice, _ = run_chain(x[None], N_CALL, inverted=inverted)
        want = oracle_stream(x, N_CALL, inverted=inverted)
        got = check_chain_channel(got_sfs[0], want)
        check_chain_voice(voice[0], want, 0)
        out.append(len(got))
    assert min(out) >= len(VOICE_PLAN) // 2, out


def test_configuration_rules_and_the_node(built):
    l = ddn.lib()
    with pytest.raises(ddn.DdnError, match=r"rc=-1 ddn_fsk4_chain_create"):
        ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_DPMR, rf_mod=2, handlers=1)
    with pytest.raises(ddn.DdnError, match=r"rc=-1 ddn_fsk4_chain_create"):
        ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_DPMR, rf_mod=2, handlers=0, inverted=2)
    dmr = ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_DMR, rf_mod=2)
    assert l.ddn_fsk4_chain_get_dpmr_results(dmr.h, C.byref(ddn.DpmrChainResults())) == -1
    dmr.close()
    # kind = DDN_NODE_FSK4 with dPMR: two parts on one device == one chain
    iq = _capture_iq()
    B, n = 4, N_CALL
    x = np.stack([np.roll(iq[:, ::-1], 911 * c, axis=0)[:2 * n] for c in range(B)])      # (negated: -fm locks on every superframe)
    one = ddn.Fsk4ChainC(B, n, ddn.FSK4_DPMR, rf_mod=2, handlers=0, vocoder=0)
    cfg = ddn.Fsk4ChainConfig(0, 0, 0, 0, ddn.FSK4_DPMR, 2, 0, 0, 0)
    node = ddn.NodeC(B, n, n_devices=2, kind=ddn.NODE_FSK4, chain_cfg=cfg, vocoder=0)
    assert node.parts == 2
    seen = 0
    for k in range(2):
        piece = np.ascontiguousarray(x[:, k * n:(k + 1) * n])
        p = _upload(l, piece)
        one.run(p)
        rd = one.dpmr_results()
        S = rd.max_syncs
        want_ns = one.fetch(rd.d_n_sync, np.int32, (B,))
        want = {name: one.fetch(getattr(rd, name), dt, (B, S) + shp) for name, dt, shp in
                (("d_fields2x8", np.int32, (2, 8)), ("d_tg", np.int32, ()), ("d_src", np.int32, ()),
                 ("d_kind", np.uint8, ()), ("d_color", np.int32, ()))}
        ptrs = []
        for q, (_, f, m) in enumerate(node.info):
            sub = np.ascontiguousarray(piece[f:f + m])
            dp = C.c_void_p()
            assert l.ddn_node_device_alloc(node.h, q, sub.nbytes, C.byref(dp)) == 0
            assert l.ddn_node_device_upload(node.h, q, dp, sub.ctypes.data, sub.nbytes) == 0
            ptrs.append(dp)
        node.run_device(ptrs)
        node.wait()
        for q, (_, f, m) in enumerate(node.info):
            a = ddn.Fsk4ChainC(m, n, 0, handle=node.chain_object(q))
            ra = a.dpmr_results()
            assert ra.max_syncs == S
            ns = a.fetch(ra.d_n_sync, np.int32, (m,))
            assert np.array_equal(ns, want_ns[f:f + m])
            for name, dt, shp in (("d_fields2x8", np.int32, (2, 8)), ("d_tg", np.int32, ()), ("d_src", np.int32, ()), ("d_kind", np.uint8, ()),
                                  ("d_color", np.int32, ())):
                g = a.fetch(getattr(ra, name), dt, (m, S) + shp)
                for c in range(m):
                    assert np.array_equal(g[c, :ns[c]], want[name][f + c, :ns[c]]), (k, q, c, name)
                    seen += int(ns[c])
        for q, dp in enumerate(ptrs):
            l.ddn_node_device_free(node.h, q, dp)
        l.ddn_device_free(p)
    assert seen > 0
    node.flush()
    node.close()
    one.close()
