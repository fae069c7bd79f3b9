"""D-STAR (-fd) on the device: DDN_FSK4_DSTAR as the fsk4 loop's seventh protocol against the profile-driven oracle loop, and the
header / voice kernels (ddn_dstar.hip) against tests/dstar.py field for field, on the reference's capture and on generated units."""
import ctypes as C

import numpy as np
import pytest

import ddn
import dstar
import rx4
from test_rx4_gpu import check_channel

pytestmark = pytest.mark.gpu
THR = np.array([0.0, 0.5, -0.5, 1.0, -1.0], np.float32)


def _batch(disc, B):
    """copies of the capture: plain, negated, delayed, after silence"""
    n = len(disc)
    rng = np.random.default_rng(5)
    x = np.zeros((B, n), np.float32)
    for c in range(B):
        d = 37 * c
        x[c, :d] = rng.standard_normal(d) * 300
        x[c, d:] = disc[:n - d]
    x[1] = -x[1]
    if B > 3:
        x[3, :20000] = 0
    return x


@pytest.mark.parametrize("cpw", [0, 1, 4])
@pytest.mark.parametrize("rf_mod", [2, 0])
def test_dstar_loop_bit_exact_with_call_splits(built, cpw, rf_mod):
    disc = rx4.capture_disc("iq_dstar.npz", 1)
    B = 4
    x = _batch(disc, B)
    n = x.shape[1]
    gpu = ddn.Fsk4Rx(B, ddn.FSK4_DSTAR, rf_mod=rf_mod, use_matched_filter=1)     # (ignored: D-STAR has no matched filter)
    if cpw:
        assert ddn.lib().ddn_fsk4_rx_set_channels_per_wave(gpu.h, cpw) == 0
    cpu = [rx4.OracleFsk4Rx(dstar.profile(rf_mod)) for _ in range(B)]
    cuts = [0, 4097, 4097 + 63, 48000, 60001, 96000 + 17, 150000, n]
    pats = [[] for _ in range(B)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        got = gpu.run_host(x[:, a:b])
        for c in range(B):
            want = cpu[c].run(x[c, a:b], max_sync=got["sync_pos"].shape[1])
            check_channel(got, c, want)
            pats[c] += want["sync_pat"].tolist()
            assert np.array_equal(gpu.thresholds(c).view(np.uint32), cpu[c].thresholds().view(np.uint32)), (c, a)
    assert dstar.PAT_HD_POS in pats[0] and dstar.PAT_VOICE_POS in pats[0]
    assert dstar.PAT_HD_NEG in pats[1] and dstar.PAT_VOICE_NEG in pats[1]


def _device_loop(x, rf_mod=2):
    import torch
    l = ddn.lib()
    B, n = x.shape
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rx = ddn.Fsk4Rx(B, ddn.FSK4_DSTAR, rf_mod=rf_mod)
    ms, my = l.ddn_fsk4_rx_max_symbols(rx.h, n), l.ddn_fsk4_rx_max_syncs(rx.h, n)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    rec, fl, pay = z((B, ms, 10), torch.uint8), z((B, ms), torch.uint8), z((B, ms, 2), torch.uint8)
    cnt, ns, spos = z((B,), torch.int32), z((B,), torch.int32), z((B, my), torch.int32)
    spat, pre, prel = z((B, my), torch.uint8), z((B, my, 90), torch.uint8), z((B, my, 90), torch.uint8)
    thr = z((B, my, 5), torch.float32)
    p = lambda t: t.data_ptr()
    assert l.ddn_fsk4_rx_set_sync_thresholds(rx.h, p(thr)) == 0
    assert l.ddn_fsk4_rx_run(rx.h, p(d), n, p(rec), p(fl), p(pay), p(cnt), ms, p(spos), p(spat), p(pre), p(prel), p(ns), my, None) == 0
    torch.cuda.synchronize()
    rx.close()
    return dict(rec=rec, cnt=cnt, ns=ns, spos=spos, spat=spat, thr=thr, ms=ms, my=my)


def _decode(o):
    """both kernels over the loop's (device) outputs -> host arrays"""
    import torch
    l = ddn.lib()
    B, my = o["spos"].shape
    z = lambda shape: torch.full(shape, 0xAB, dtype=torch.uint8, device="cuda")    # poison: every slot must be written
    h41, hok, hv = z((B, my, 41)), z((B, my)), z((B, my))
    am, sdb, kind, sh41, sok, stx, vv = z((B, my, 21, 4, 24)), z((B, my, 60)), z((B, my)), z((B, my, 41)), z((B, my)), z((B, my, 60)), z((B, my))
    p = lambda t: t.data_ptr()
    args = (p(o["rec"]), o["rec"].shape[1], p(o["cnt"]), p(o["spos"]), p(o["spat"]), p(o["ns"]), p(o["thr"]), B, my)
    assert l.ddn_dstar_header_decode_batch(*args, p(h41), p(hok), p(hv), None) == 0
    assert l.ddn_dstar_voice_decode_batch(*args, p(am), p(sdb), p(kind), p(sh41), p(sok), p(stx), p(vv), None) == 0
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()
    return dict(h41=h(h41), hok=h(hok), hv=h(hv), ambe=h(am), sdb=h(sdb), kind=h(kind), sh41=h(sh41), sok=h(sok), text=h(stx), vv=h(vv))


def _symbols(rec_row, k):
    return rec_row[:k, 6:10].copy().view(np.float32).reshape(-1)


def _check_slots(o, got):
    """every slot of every channel against the restatement on the same records and thresholds"""
    rec, cnt, ns = o["rec"].cpu().numpy(), o["cnt"].cpu().numpy(), o["ns"].cpu().numpy()
    spos, spat, thr = o["spos"].cpu().numpy(), o["spat"].cpu().numpy(), o["thr"].cpu().numpy()
    B, my = spos.shape
    n_hdr = n_voice = 0
    for c in range(B):
        sym = _symbols(rec[c], int(cnt[c]))
        for k in range(my):
            hv = vv = False
            if k < ns[c]:
                a, pat = int(spos[c, k]) + 1, int(spat[c, k])
                hv = pat >= 2 and a + dstar.HEADER_SYMS <= len(sym)
                off = dstar.HEADER_SYMS if pat >= 2 else 0
                vv = a + off + dstar.VOICE_SYMS <= len(sym)
            assert got["hv"][c, k] == hv and got["vv"][c, k] == vv, (c, k)
            if hv:
                h, ok = dstar.decode_header(sym[a:a + dstar.HEADER_SYMS], thr[c, k])
                assert bytes(got["h41"][c, k]) == bytes(h) and got["hok"][c, k] == ok, (c, k)
                n_hdr += 1
            else:
                assert not got["h41"][c, k].any() and got["hok"][c, k] == 0
            if vv:
                fr, sd = dstar.voice_gather(dstar.bits2(sym[a + off:a + off + dstar.VOICE_SYMS], thr[c, k, 0], pat & 1))
                s = dstar.slow_data(sd)
                assert np.array_equal(got["ambe"][c, k], fr), (c, k)
                assert bytes(got["sdb"][c, k]) == s["bytes"] and got["kind"][c, k] == s["kind"], (c, k)
                assert bytes(got["sh41"][c, k]) == s["hdr41"] and got["sok"][c, k] == s["crc_ok"], (c, k)
                assert bytes(got["text"][c, k]) == (s["text"] or bytes(60)), (c, k)
                n_voice += 1
            else:
                assert not got["ambe"][c, k].any() and not got["sdb"][c, k].any() and got["kind"][c, k] == 0
    return n_hdr, n_voice


@pytest.mark.parametrize("rf_mod", [2, 0])
def test_dstar_kernels_on_the_capture_give_src_kb7wuk(built, rf_mod):
    """DECODE_IQ_DSTAR (tests/CMakeLists.txt:8951): "SRC: KB7WUK" from the device, on plain, negated and delayed copies"""
    disc = rx4.capture_disc("iq_dstar.npz", 1)
    x = _batch(disc, 3)
    o = _device_loop(x, rf_mod)
    # the thresholds each sync left are the oracle loop's
    for c in range(3):
        want = rx4.OracleFsk4Rx(dstar.profile(rf_mod)).run(x[c])
        ns = int(o["ns"][c])
        assert np.array_equal(o["spos"][c, :ns].cpu().numpy(), want["sync_pos"])
        assert np.array_equal(o["thr"][c, :ns].cpu().numpy().view(np.uint32), want["sync_thr"].view(np.uint32))
    got = _decode(o)
    n_hdr, n_voice = _check_slots(o, got)
    assert n_hdr >= 6 and n_voice >= 9, (n_hdr, n_voice)
    for c in range(3):
        srcs = [bytes(got["sh41"][c, k, 27:39]).decode("latin-1") for k in range(int(o["ns"][c]))
                if got["vv"][c, k] and got["kind"][c, k] == dstar.SD_HEADER and got["sok"][c, k]]
        assert len(srcs) >= 3 and all(s.startswith("KB7WUK") for s in srcs), (c, srcs)


def _generated(rng, B=4, n=30000):
    """records with generated units (both polarities, header and voice syncs, flipped coded bits, bad CRCs, text and header slow data,
    units that end past the call) between noise; -> the loop's output layout as torch tensors + what was sent"""
    import torch
    my = 12
    sym = (rng.standard_normal((B, n)) * 0.6).astype(np.float32)
    spos, spat, ns = np.zeros((B, my), np.int32), np.zeros((B, my), np.uint8), np.zeros(B, np.int32)
    thr = np.zeros((B, my, 5), np.float32)
    cnt = np.full(B, n, np.int32)
    cnt[3] = n - 1500                         # the last units of channel 3 end past its call
    w, x, _ = dstar._tables()
    mask = np.zeros((4, 24), bool)
    mask[w, x] = True
    for c in range(B):
        at, k = 100 + 17 * c, 0
        while at + 2700 < n and k < my:
            pat = int(rng.integers(0, 4))
            neg = pat & 1
            lvl, ctr = float(rng.uniform(0.5, 2.0)), float(rng.uniform(-0.2, 0.2))
            units = []
            if pat >= 2:
                h = dstar.make_header(int(rng.integers(0, 256)), "RPT%d" % k, "GW%d" % c, "CQCQCQ", "KB7WUK  ID%02d" % k,
                                      good_crc=bool(rng.integers(0, 4)))
                a = dstar.encode_header(h)
                flips = rng.choice(660, int(rng.integers(0, 12)), replace=False)
                a[flips] ^= 1
                units.append(np.where(a == 1, ctr + lvl, ctr - lvl).astype(np.float32))
            fr = rng.integers(0, 2, (21, 4, 24)).astype(np.uint8)
            fr[:, ~mask] = 0
            m = int(rng.integers(0, 4))
            if m == 0:
                sdb = dstar.compact_to_sd_bytes(dstar.make_header(0, "A", "B", "C", "N0CALL %d" % k, good_crc=bool(rng.integers(0, 2))), 0x55)
            elif m == 1:
                sdb = bytes([0x40]) + b"HELLO xWORLD  \x01ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789abcdefghijklmnopq"[:59]
            elif m == 2:
                sdb = bytes([0x35]) + (b"$$CRC" if rng.integers(0, 2) else b"TEXT!") + bytes(rng.integers(0, 256, 54).astype(np.uint8))
            else:
                sdb = bytes(rng.integers(0, 256, 60).astype(np.uint8))
            v = dstar.encode_voice(fr, dstar.encode_slow_data(sdb))
            units.append(dstar.bits_to_symbols(v, neg, lvl, ctr, rng, 0.3 * lvl))
            u = np.concatenate(units)
            spos[c, k], spat[c, k] = at - 1, pat
            thr[c, k] = [ctr, ctr + 0.6 * lvl, ctr - 0.6 * lvl, ctr + lvl * float(rng.uniform(0.8, 1.2)), ctr - lvl * float(rng.uniform(0.8, 1.2))]
            if k == 2:
                thr[c, k, 3:] = thr[c, k, 0]          # degenerate thresholds: the cost's fallback span
            m_ = min(len(u), n - at)
            sym[c, at:at + m_] = u[:m_]
            at += len(u) + int(rng.integers(-300, 400))    # (a negative gap: the next sync lies inside this unit)
            k += 1
        ns[c] = k
    rec = np.zeros((B, n, 10), np.uint8)
    rec[:, :, 6:10] = sym.view(np.uint8).reshape(B, n, 4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(rec=t(rec), cnt=t(cnt), ns=t(ns), spos=t(spos), spat=t(spat), thr=t(thr))


def test_dstar_kernels_on_generated_units(built):
    rng = np.random.default_rng(2026)
    o = _generated(rng)
    got = _decode(o)
    n_hdr, n_voice = _check_slots(o, got)
    assert n_hdr >= 8 and n_voice >= 20, (n_hdr, n_voice)
    assert got["hok"].astype(bool).sum() >= 4 and (got["hv"].astype(bool) & ~got["hok"].astype(bool)).sum() >= 1
    kinds = set(got["kind"][got["vv"].astype(bool)].tolist())
    assert {1, 2, 3} <= kinds


def test_dstar_abi(built):
    l = ddn.lib()
    for name in ("ddn_dstar_header_decode_batch", "ddn_dstar_voice_decode_batch"):
        assert hasattr(l, name)
    with pytest.raises(ddn.DdnError, match=r"rc=-1 ddn_fsk4_rx_create: bad configuration"):
        ddn.Fsk4Rx(2, ddn.FSK4_DSTAR, inverted=1)         # DDN_EINVAL: D-STAR hunts both polarities
    with pytest.raises(ddn.DdnError, match=r"rc=-1 ddn_fsk4_rx_create: bad configuration"):
        ddn.Fsk4Rx(2, ddn.FSK4_DSTAR, rf_mod=1)
    b = ddn.Fsk4Rx(2, ddn.FSK4_DSTAR)
    assert l.ddn_fsk4_rx_set_handlers(b.h, 1) == -1       # fixed counts, no handler family
    b.close()
    assert l.ddn_dstar_header_decode_batch(None, 0, None, None, None, None, None, -1, 1, None, None, None, None) == -1
    assert l.ddn_dstar_voice_decode_batch(None, 0, None, None, None, None, None, 1, 1, *([None] * 7), None) == -1
