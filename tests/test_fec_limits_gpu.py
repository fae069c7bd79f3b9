"""GPU: the size limits and small-batch edges of the FEC decoders' dense public forms against the oracle, bit-exact: the NXDN
convolution's n_steps limit (decided on the host against the LDS a workgroup may have - the test reads the same figure from the device
properties and never tries a launch the entry has not checked), its n_bits / out_stride / batch edges, the K = 5 libM17 decoder's
puncture and length edges and refusals, the trellis and block-code kernels at their workgroup edges, and n = 0 everywhere."""
import ctypes as C

import numpy as np
import pytest

import bptc_small as bs
import ddn
import fec3
import fec_edge as fe
import fecgen

pytestmark = pytest.mark.gpu


def _limit():
    import torch
    return int(torch.cuda.get_device_properties(0).shared_memory_per_block)


def nxdn_host(sym, rel, steps, nbits, m0, stride=None):
    n = sym.shape[0]
    stride = (nbits + 7) // 8 if stride is None else stride
    out = fe.sentinel((n, max(stride, 1)))
    m = None if m0 is None else m0.copy()
    rc = ddn.lib().ddn_fec_nxdn_conv_host(sym.ctypes.data, rel.ctypes.data if rel is not None else None, n, steps, nbits,
                                          m.ctypes.data if m is not None else None, out.ctypes.data, stride)
    return rc, out, m


@pytest.mark.parametrize("soft", [0, 1])
def test_nxdn_conv_n_steps_limit(built, soft):
    """the largest n_steps <= 1024 whose 16 code words fit the device's LDS per workgroup decodes like the oracle (hard and soft, metrics
    carried); the first that does not fit is refused with DDN_ERANGE, out and metrics_io untouched.  On gfx950 (160 KiB) 1024 fits both
    forms - 65,584 and 98,384 bytes, above the 64 KiB a kernel has without opting in - and equality at 1024 is the whole check."""
    limit = _limit()
    top = max(s for s in range(1, 1025) if fe.nxdn_lds_bytes(s, soft) <= limit)
    print("LDS per workgroup %d bytes; soft %d: largest n_steps %d needs %d" % (limit, soft, top, fe.nxdn_lds_bytes(top, soft)))
    n = 17
    sym, rel, m0 = fe.nxdn_inputs(n, top)
    rel = rel if soft else None
    rc, out, m = nxdn_host(sym, rel, top, top - 4, m0)
    assert rc == ddn.DDN_OK, ddn.lib().ddn_last_error()
    wo, wm = fecgen.oracle_nxdn(sym, rel, top, top - 4, metrics=m0)
    assert np.array_equal(out, wo) and np.array_equal(m, wm)
    if top < 1024:
        sym2, rel2, _ = fe.nxdn_inputs(n, top + 1)
        rc, out, m = nxdn_host(sym2, rel2 if soft else None, top + 1, top - 3, m0)
        assert rc == ddn.DDN_ERANGE and b"LDS" in ddn.lib().ddn_last_error()
        assert fe.untouched(out) and np.array_equal(m, m0)


@pytest.mark.parametrize("soft", [0, 1])
def test_nxdn_conv_edges(built, soft):
    """n_steps 1 with 0 and 1 bits, n_bits = n_steps, n_bits % 8 in {0, 1, 7}, batches around the 16 code words of a workgroup; on
    device buffers an out_stride two bytes larger than needed leaves those bytes (and the row behind the batch) as they were"""
    import torch
    l = fe.dev()
    for steps, nbits in ((1, 0), (1, 1), (40, 40), (40, 32), (40, 33), (40, 39), (9, 9)):
        N = 17
        sym, rel, m0 = fe.nxdn_inputs(N, steps, seed=nbits)
        rel = rel if soft else None
        nby = (nbits + 7) // 8
        wo, wm = fecgen.oracle_nxdn(sym, rel, steps, nbits, metrics=m0)
        for n in (1, 15, 16, 17):
            rc, out, m = nxdn_host(sym[:n], rel[:n] if soft else None, steps, nbits, m0[:n])
            assert rc == ddn.DDN_OK, ddn.lib().ddn_last_error()
            assert np.array_equal(out[:, :nby], wo[:n]) and np.array_equal(m, wm[:n]), (steps, nbits, n)
            d_sym = torch.from_numpy(np.ascontiguousarray(sym[:n])).cuda()
            d_rel = torch.from_numpy(np.ascontiguousarray(rel[:n])).cuda() if soft else None
            d_out = torch.from_numpy(fe.sentinel((n + 1, nby + 2))).cuda()
            mh = fe.sentinel((n + 1, 16), np.uint16)
            mh[:n] = m0[:n]
            d_m = torch.from_numpy(mh).cuda()
            assert l.ddn_fec_nxdn_conv_batch(d_sym.data_ptr(), d_rel.data_ptr() if soft else None, n, steps, nbits, d_m.data_ptr(),
                                             d_out.data_ptr(), nby + 2, None) == 0, l.ddn_last_error()
            torch.cuda.synchronize()
            got, gm = d_out.cpu().numpy(), d_m.cpu().numpy()
            assert np.array_equal(got[:n, :nby], wo[:n]) and fe.untouched(got[:n, nby:]) and fe.untouched(got[n]), (steps, nbits, n)
            assert np.array_equal(gm[:n], wm[:n]) and fe.untouched(gm[n]), (steps, nbits, n)
    # refusals that never reach the device: more bits than steps, no steps, too many steps, a stride too small
    sym, rel, m0 = fe.nxdn_inputs(2, 40)
    for steps, nbits, stride in ((40, 41, 6), (0, 0, 1), (1025, 8, 1), (40, 33, 4)):
        out = fe.sentinel((2, 8))
        m = m0.copy()
        rc = ddn.lib().ddn_fec_nxdn_conv_host(sym.ctypes.data, None, 2, steps, nbits, m.ctypes.data, out.ctypes.data, stride)
        assert rc == ddn.DDN_EINVAL and fe.untouched(out) and np.array_equal(m, m0), (steps, nbits, stride)


def m17_host(soft, punct, stride, with_cost=True):
    n, in_len = soft.shape
    out = fe.sentinel((n, stride))
    cost = fe.sentinel((n,), np.uint32)
    rc = ddn.lib().ddn_fec_viterbi_k5_host(soft.ctypes.data, n, in_len, punct.ctypes.data if punct is not None else None,
                                           len(punct) if punct is not None else 0, out.ctypes.data, stride,
                                           cost.ctypes.data if with_cost else None)
    return rc, out, cost


@pytest.mark.parametrize("case", range(len(fe.K5_CASES)))
def test_viterbi_k5_puncture_and_length_edges(built, case):
    """p_len 1 and 64, patterns that start with 0, an in_len that ends inside a period (the cost of the erased soft bits), odd in_len and
    odd depunctured lengths, exactly 488 depunctured soft bits; an out_stride three bytes larger than needed reads zeros there; cost NULL.
    (The walk that sizes the depunctured word ends on a kept soft bit, so inside it every kept place has a received soft bit: the
    kernel's `i < in_len` guard never fails there, and the erased places are the pattern's zeros - their 0x7FFF each is what the
    reported cost takes off again.)"""
    in_len, punct, u_len = fe.K5_CASES[case]
    soft = fecgen.gen_m17(np.random.default_rng(fe.FZ + 70 + case), 17, in_len, sigma=20000.0)
    wo, wc, need = fecgen.oracle_m17(soft, punct)
    assert need == (u_len // 2 + 3) // 8 + 1
    for n in (1, 15, 16, 17):
        rc, out, cost = m17_host(soft[:n], punct, need + 3)
        assert rc == ddn.DDN_OK, ddn.lib().ddn_last_error()
        assert np.array_equal(out[:, :need], wo[:n]) and not out[:, need:].any() and np.array_equal(cost, wc[:n]), (case, n)
    rc, out, cost = m17_host(soft, punct, need, with_cost=False)
    assert rc == ddn.DDN_OK and np.array_equal(out, wo) and fe.untouched(cost)
    rc, out, cost = m17_host(soft, punct, need - 1)                       # a stride one byte short
    assert rc == ddn.DDN_EINVAL and fe.untouched(out) and fe.untouched(cost)


def test_viterbi_k5_refusals(built):
    """489 and 490 depunctured soft bits (one and two above the 244-step history), a pattern of zeros, a pattern of 65 entries"""
    for in_len, punct, u_len in fe.K5_TOO_LONG:
        soft = fecgen.gen_m17(np.random.default_rng(fe.FZ + 80), 3, in_len)
        rc, out, cost = m17_host(soft, punct, 40)
        assert rc == ddn.DDN_ERANGE and fe.untouched(out) and fe.untouched(cost), u_len
    soft = fecgen.gen_m17(np.random.default_rng(fe.FZ + 81), 3, 96)
    rc, out, cost = m17_host(soft, np.zeros(4, np.uint8), 40)
    assert rc == ddn.DDN_EINVAL and fe.untouched(out) and fe.untouched(cost)
    rc, out, cost = m17_host(soft, np.ones(65, np.uint8), 40)
    assert rc == ddn.DDN_ERANGE and fe.untouched(out) and fe.untouched(cost)


def test_trellis_hosts_at_their_group_edges(built):
    """k_p25_half_rate: 64 code words per workgroup, metric NULL allowed; k_r34: 32 per workgroup, hard and weighted"""
    l = ddn.lib()
    llr = fe.half_inputs(65)
    wo, wm = fecgen.oracle_p25_half_rate(llr)
    for n in (1, 63, 64, 65):
        out, met = fe.sentinel((n, 12)), fe.sentinel((n,), np.int32)
        assert l.ddn_fec_p25_12_soft_host(llr.ctypes.data, n, out.ctypes.data, met.ctypes.data) == 0
        assert np.array_equal(out, wo[:n]) and np.array_equal(met, wm[:n]), n
        out = fe.sentinel((n, 12))
        assert l.ddn_fec_p25_12_soft_host(llr.ctypes.data, n, out.ctypes.data, None) == 0
        assert np.array_equal(out, wo[:n]), n
    d, rel = fe.r34_inputs(33)
    for r in (None, rel):
        want = fecgen.oracle_r34(d, r)
        for n in (1, 31, 32, 33):
            out = fe.sentinel((n, 18))
            assert l.ddn_fec_r34_host(d.ctypes.data, r.ctypes.data if r is not None else None, n, out.ctypes.data) == 0
            assert np.array_equal(out, want[:n]), n


def test_block_codes_at_their_group_edges(built):
    """k_block_code (256 threads) at n 1 / 255 / 256 / 257 for every code; the BPTC and RS(12,9) kernels (128 threads) at 1 / 127 / 128 /
    129 - the existing tests start at n = 2000"""
    l = ddn.lib()
    rng = np.random.default_rng(fe.FZ + 90)
    for code, (nb, k, _) in fec3.CODES.items():
        words = rng.integers(0, 2, (257, nb), dtype=np.uint8)
        words[::3] = 0
        for i in range(0, 257, 3):
            words[i, rng.integers(0, nb)] = 1
        ww, wd, wk = fec3.oracle_decode(code, words)
        for n in (1, 255, 256, 257):
            w, dec, ok = words[:n].copy(), fe.sentinel((n, k)), fe.sentinel((n,))
            assert l.ddn_fec_block_code_host(code, w.ctypes.data, n, 1, dec.ctypes.data, ok.ctypes.data) == 0
            assert np.array_equal(w, ww[:n]) and np.array_equal(ok, wk[:n]), (code, n)
            if 1 <= code <= 4:                       # (only the Hamming decoders with a codeword count write `decoded`)
                done = wk[:n].astype(bool) | (code == 1)
                assert np.array_equal(dec[done], wd[:n][done]), (code, n)
            else:
                assert fe.untouched(dec), (code, n)
    x = fec3.bptc_inputs(rng, 129)
    wo, wr, we = fec3.oracle_bptc(x, 0)
    cs = bs.cases128(rng, 129)
    x128 = np.stack(cs).reshape(len(cs), 128)[:129]
    w128 = [bs.oracle_128x77(m) for m in cs[:129]]
    x32 = np.stack([bs.word32(rng, i % 4, 1) if i % 5 else rng.integers(0, 4, 32).astype(np.uint8) for i in range(129)])
    w32 = [bs.oracle_16x2(v, 1) for v in x32]
    o = fec3.orc.oracle()
    cw = rng.integers(0, 256, (129, 12)).astype(np.uint8)
    cw[::2] = 0
    for i in range(0, 129, 2):
        e = int(rng.integers(0, 3))
        cw[i, rng.choice(12, e, replace=False)] = rng.integers(1, 256, e)
    wcw, wres, wf, wsyn = cw.copy(), np.zeros(129, np.uint8), np.zeros(129, np.uint8), np.zeros((129, 3), np.uint8)
    for i in range(129):
        f = C.c_uint8(0)
        wres[i] = o.orc_rs_12_9(C.c_void_p(wcw[i].ctypes.data), C.c_void_p(wsyn[i].ctypes.data), C.byref(f))
        wf[i] = f.value
    for n in (1, 127, 128, 129):
        out, r3, e = fe.sentinel((n, 96)), fe.sentinel((n, 3)), fe.sentinel((n,), np.uint32)
        assert l.ddn_fec_bptc_196x96_host(x.ctypes.data, 0, n, out.ctypes.data, r3.ctypes.data, e.ctypes.data) == 0
        assert np.array_equal(out, wo[:n]) and np.array_equal(r3, wr[:n]) and np.array_equal(e, we[:n]), n
        out, e = fe.sentinel((n, 77)), fe.sentinel((n,), np.uint32)
        assert l.ddn_fec_bptc_128x77_host(x128.ctypes.data, n, out.ctypes.data, e.ctypes.data) == 0
        assert all(e[i] == w128[i][0] and np.array_equal(out[i], w128[i][1]) for i in range(n)), n
        out, e = fe.sentinel((n, 32)), fe.sentinel((n,), np.uint32)
        assert l.ddn_fec_bptc_16x2_host(x32.ctypes.data, n, 1, out.ctypes.data, e.ctypes.data) == 0
        assert all(e[i] == w32[i][0] and np.array_equal(out[i], w32[i][1]) for i in range(n)), n
        got, res, fnd, syn = cw[:n].copy(), fe.sentinel((n,)), fe.sentinel((n,)), fe.sentinel((n, 3))
        assert l.ddn_fec_rs_12_9_host(got.ctypes.data, n, res.ctypes.data, fnd.ctypes.data, syn.ctypes.data) == 0
        assert np.array_equal(got, wcw[:n]) and np.array_equal(res, wres[:n]) and np.array_equal(fnd, wf[:n]), n
        assert np.array_equal(syn, wsyn[:n]), n


def test_n_zero_is_ok_and_writes_nothing(built):
    l = ddn.lib()
    a = fe.sentinel((4096,))          # one buffer stands for every argument: with n = 0 nothing may be read or written
    p = a.ctypes.data
    one = np.array([1], np.uint8)
    calls = [
        lambda: l.ddn_fec_p25_12_soft_host(p, 0, p, p),
        lambda: l.ddn_fec_r34_host(p, p, 0, p),
        lambda: l.ddn_fec_nxdn_conv_host(p, p, 0, 40, 36, p, p, 5),
        lambda: l.ddn_fec_viterbi_k5_host(p, 0, 96, one.ctypes.data, 1, p, 7, p),
        lambda: l.ddn_fec_p25_12_soft_list_host(p, 0, 8, p, p),
        lambda: l.ddn_fec_r34_list_host(p, p, 0, 32, p, p),
        lambda: l.ddn_fec_p25_mbf34_list_host(p, 0, 8, p, p),
        lambda: l.ddn_fec_block_code_host(0, p, 0, 1, p, p),
        lambda: l.ddn_fec_bptc_196x96_host(p, 0, 0, p, p, p),
        lambda: l.ddn_fec_bptc_128x77_host(p, 0, p, p),
        lambda: l.ddn_fec_bptc_16x2_host(p, 0, 1, p, p),
        lambda: l.ddn_fec_rs_12_9_host(p, 0, p, p, p),
    ]
    for k, call in enumerate(calls):
        assert call() == ddn.DDN_OK, (k, l.ddn_last_error())
        assert fe.untouched(a), k
