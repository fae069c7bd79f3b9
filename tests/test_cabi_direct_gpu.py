"""GPU: entry points of the C ABI that no other test calls by name (tests/test_cabi_called.py keeps every exported function reached
by a test): the block-code drop-ins with the reference's names, the soft step of the NXDN convolutional drop-in, the timing and
counter getters of the receive loops and of the vocoder, two accessors of the chain objects, and the device-pointer variant of the
small BPTC."""
import ctypes as C

import numpy as np
import pytest

import ddn
import fec3
import fecgen
import mbe
import orc
from test_mbe_gpu import GpuVocoder

pytestmark = pytest.mark.gpu


def test_block_code_dropins_by_name(built):
    """every *_init is callable (the tables are compile-time here) and every *_decode equals the restatement on sixty words drawn from
    all words of the code's length (code words, correctable and uncorrectable ones); the Hamming(12,8) .. (16,11,4) forms also
    return the data bits"""
    l = ddn.lib()
    table = {0: (l.Hamming_7_4_init, l.Hamming_7_4_decode), 1: (l.Hamming_12_8_init, l.Hamming_12_8_decode),
             2: (l.Hamming_13_9_init, l.Hamming_13_9_decode), 3: (l.Hamming_15_11_init, l.Hamming_15_11_decode),
             4: (l.Hamming_16_11_4_init, l.Hamming_16_11_4_decode), 5: (l.Golay_20_8_init, l.Golay_20_8_decode),
             7: (l.QR_16_7_6_init, l.QR_16_7_6_decode)}
    rng = np.random.default_rng(12)
    for code, (init, decode) in table.items():
        n, k, name = fec3.CODES[code]
        assert init() is None
        pool = fec3.words_for(code, rng)
        words = pool[rng.integers(0, len(pool), 60)].copy()
        want_w, want_d, want_ok = fec3.oracle_decode(code, words)
        for i in range(len(words)):
            g, dec = words[i].copy(), np.zeros(k, np.uint8)
            got = decode(g.ctypes.data, dec.ctypes.data, 1) if 1 <= code <= 4 else decode(g.ctypes.data)
            assert bool(got) == bool(want_ok[i]) and np.array_equal(g, want_w[i]), (name, i)
            if 1 <= code <= 4 and want_ok[i]:
                assert np.array_equal(dec, want_d[i]), (name, i)
        assert want_ok.any() and not np.array_equal(want_w, words)                         # words were accepted, bits were corrected


def test_nxdn_convolution_soft_step(built):
    """CNXDNConvolution_decode_soft: the streaming decode with reliabilities equals the restatement's soft decode, metrics carried
    from one frame to the next, and differs from the hard decode of the same symbols somewhere"""
    l = ddn.lib()
    rng = np.random.default_rng(44)
    sym, rel = fecgen.gen_nxdn(rng, 6, 96, p_err=0.09, random_frac=0.0)
    l.CNXDNConvolution_init()
    m = np.zeros((1, 16), np.uint16)
    differs = 0
    for i in range(len(sym)):
        l.CNXDNConvolution_start()
        for t in range(96):
            l.CNXDNConvolution_decode_soft(int(sym[i, 2 * t]), int(sym[i, 2 * t + 1]), int(rel[i, 2 * t]), int(rel[i, 2 * t + 1]))
        o = np.full(12, 0xFF, np.uint8)
        l.CNXDNConvolution_chainback(o.ctypes.data, 92)
        hard, _ = fecgen.oracle_nxdn(sym[i:i + 1], None, 96, 92, metrics=m)
        wo, m = fecgen.oracle_nxdn(sym[i:i + 1], rel[i:i + 1], 96, 92, metrics=m)
        assert np.array_equal(o[:11], wo[0, :11]) and (o[11] >> 4) == (wo[0, 11] >> 4) and (o[11] & 0x0F) == 0x0F, i
        differs += not np.array_equal(hard, wo)
    assert differs > 0


def test_p25_rx_timing_and_counters(built):
    l = ddn.lib()
    B, n = 9, 6000
    x = orc.synth_p25_disc(61, B, n, frame_dibits=432)[0]
    plain = ddn.P25Rx(B, lock_symbols=408).run(x)
    rx = ddn.P25Rx(B, lock_symbols=408)
    ms, k = np.full(2, -1.0, np.float32), C.c_int(-1)
    assert l.ddn_p25_rx_get_timing(rx.h, ms.ctypes.data) == ddn.DDN_EINVAL             # never switched on
    assert l.ddn_p25_rx_set_timing(rx.h, 1) == 0
    assert l.ddn_p25_rx_get_timing_avg(rx.h, ms.ctypes.data, C.byref(k)) == 0 and k.value == 0 and not ms.any()
    halves = [rx.run(x[:, :n // 2]), rx.run(x[:, n // 2:])]
    assert l.ddn_p25_rx_get_timing(rx.h, ms.ctypes.data) == 0 and np.isfinite(ms).all() and (ms >= 0).all() and ms[1] > 0
    assert l.ddn_p25_rx_get_timing_avg(rx.h, ms.ctypes.data, C.byref(k)) == 0 and k.value == 2
    assert np.isfinite(ms).all() and (ms >= 0).all() and ms[1] > 0
    assert l.ddn_p25_rx_set_timing(rx.h, 0) == 0 and l.ddn_p25_rx_set_timing(None, 1) == ddn.DDN_EINVAL
    assert l.ddn_p25_rx_get_timing_avg(rx.h, ms.ctypes.data, None) == ddn.DDN_EINVAL
    for c in range(B):                                   # timing on changes nothing of what the loop writes
        kk = int(plain[2][c])
        assert kk == halves[0][2][c] + halves[1][2][c]
        got = np.concatenate([h[0][c, :h[2][c]] for h in halves])
        assert np.array_equal(got, plain[0][c, :kk]), c
    out2 = (C.c_longlong * 2)(-1, -1)
    assert l.ddn_p25_rx_debug_counters(rx.h, 0, out2) == 0 and out2[0] >= 0 and out2[1] >= 0
    assert l.ddn_p25_rx_debug_counters(rx.h, B, out2) == ddn.DDN_EINVAL and l.ddn_p25_rx_debug_counters(rx.h, 0, None) == ddn.DDN_EINVAL


def test_fsk4_rx_timing(built):
    import rx4
    l = ddn.lib()
    disc = rx4.capture_disc("iq_nxdn48.npz", 1)[60000:72000]
    x = np.stack([disc, -disc]).astype(np.float32)
    plain = ddn.Fsk4Rx(2, ddn.FSK4_NXDN48).run_host(x)
    rx = ddn.Fsk4Rx(2, ddn.FSK4_NXDN48)
    ms = np.full(2, -1.0, np.float32)
    assert l.ddn_fsk4_rx_get_timing(rx.h, ms.ctypes.data) == ddn.DDN_EINVAL            # never switched on
    assert l.ddn_fsk4_rx_set_timing(rx.h, 1) == 0
    got = rx.run_host(x)
    assert l.ddn_fsk4_rx_get_timing(rx.h, ms.ctypes.data) == 0 and np.isfinite(ms).all() and (ms >= 0).all() and ms[1] > 0
    assert l.ddn_fsk4_rx_set_timing(rx.h, 0) == 0 and l.ddn_fsk4_rx_set_timing(None, 1) == ddn.DDN_EINVAL
    assert l.ddn_fsk4_rx_get_timing(rx.h, None) == ddn.DDN_EINVAL
    for key in plain:
        assert np.array_equal(plain[key], got[key]), key
    assert (got["n_sync"] > 0).all()


def test_mbe_batch_timing(built):
    l = ddn.lib()
    rng = np.random.default_rng(8)
    bits = mbe.random_imbe_bits(rng, (4, 6))
    plain, _ = GpuVocoder(ddn.MBE_IMBE, 4).run(bits)
    g = GpuVocoder(ddn.MBE_IMBE, 4)
    ms = np.full(2, -1.0, np.float32)
    assert l.ddn_mbe_batch_get_timing(g.h, ms.ctypes.data) == 0 and not ms.any()       # nothing timed yet
    assert l.ddn_mbe_batch_set_timing(g.h, 1) == 0
    got, _ = g.run(bits)
    assert l.ddn_mbe_batch_get_timing(g.h, ms.ctypes.data) == 0 and np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0
    assert l.ddn_mbe_batch_set_timing(g.h, 0) == 0 and l.ddn_mbe_batch_set_timing(None, 1) == ddn.DDN_EINVAL
    assert l.ddn_mbe_batch_get_timing(g.h, None) == ddn.DDN_EINVAL
    assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


def test_chain_accessors(built):
    """ddn_fsk4_chain_front_end hands out the chain's own ddn_batch (its filter is the one the chain's sample rate and protocol
    select); ddn_p25_chain_d2h_route names how results leave the device: 0 = plain copies, else an engine mask or 0x10000"""
    l = ddn.lib()
    ch = ddn.Fsk4ChainC(2, 4096, ddn.FSK4_NXDN48)
    fe = l.ddn_fsk4_chain_front_end(ch.h)
    assert fe and l.ddn_fsk4_chain_front_end(None) is None
    t = np.zeros(160, np.float32)
    nt = l.ddn_batch_get_taps(C.c_void_p(fe), t.ctypes.data, 160)
    designs = []
    for profile in range(6):                             # the handle is a ddn_batch: its filter is one of the reference's designs
        want = np.zeros(144, np.float32)
        nw = orc.oracle().orc_channel_lpf_design(48000, profile, want.ctypes.data, 144)
        designs.append(nt == nw and np.array_equal(t[:nt].view(np.uint32), want[:nw].view(np.uint32)))
    assert nt > 0 and any(designs)
    ch.close()
    p = ddn.P25ChainC(2, 4096)
    route = l.ddn_p25_chain_d2h_route(p.h)
    assert route == 0 or route == 0x10000 or 0 < route < 0x10000
    assert l.ddn_p25_chain_d2h_route(None) == 0
    p.close()


@pytest.mark.parametrize("odd", [0, 1])
def test_bptc_16x2_on_device_pointers(built, odd):
    import torch
    l = ddn.lib()
    rng = np.random.default_rng(3 + odd)
    n = 300
    x = rng.integers(0, 2, (n, 32), dtype=np.uint8)
    out_h, err_h = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint32)
    assert l.ddn_fec_bptc_16x2_host(x.ctypes.data, n, odd, out_h.ctypes.data, err_h.ctypes.data) == 0
    d = torch.from_numpy(x).cuda()
    out_d = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    err_d = torch.zeros(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert l.ddn_fec_bptc_16x2_batch(d.data_ptr(), n, odd, out_d.data_ptr(), err_d.data_ptr(), s.cuda_stream) == 0
    s.synchronize()
    assert np.array_equal(out_d.cpu().numpy(), out_h) and np.array_equal(err_d.cpu().numpy().view(np.uint32), err_h)
    assert l.ddn_fec_bptc_16x2_batch(None, n, odd, out_d.data_ptr(), err_d.data_ptr(), None) != 0
