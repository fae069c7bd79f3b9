"""GPU: the size limits and small-batch edges of the FEC decoders' dense public forms against the oracle, bit-exact: the NXDN
convolution's n_steps limit (decided on the host against the LDS a workgroup may have - the test reads the same figure from the device
properties and never tries a launch the entry has not checked), its n_bits / out_stride / batch edges, the K = 5 libM17 decoder's
puncture and length edges and refusals, the trellis and block-code kernels at their workgroup edges, the Reed-Solomon / Golay / soft Hamming
kernels and the Phase 2 burst stages at theirs, and n = 0 everywhere."""
import ctypes as C

import numpy as np
import pytest

import bptc_small as bs
import ddn
import fec3
import fec_edge as fe
import fecgen
import rs28

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


RS_ID = {"24_12_13": 0, "24_16_9": 1, "36_20_17": 2}


def _classes(rc_ok, changed):
    """how many clean, corrected and failed words a batch holds"""
    return int((rc_ok & ~changed).sum()), int((rc_ok & changed).sum()), int((~rc_ok).sum())


def test_rs_and_golay_hosts_at_their_group_edges(built):
    """the 64-thread kernels (k_rs63, k_rs63_soft, k_rs28_decode, k_golay24) at n 1 / 63 / 64 / 65, clean, correctable and
    uncorrectable words in every batch of 63 and more; word 0 of the soft RS batch is one that only an erasure retry decodes -
    the existing tests start at n = 1500"""
    from test_oracle_rs import gen_rs_soft, oracle_golay, oracle_rs, oracle_rs_soft_rel
    from test_rs28_gpu import _batch
    l = ddn.lib()
    N = 65
    for code, cid in RS_ID.items():
        rng = np.random.default_rng(fe.FZ + 100 + cid)
        d, p = fecgen.gen_p25_rs(rng, code, N, max_extra=4)
        d[1::9] = rng.integers(0, 2, d[1::9].shape)
        p[1::9] = rng.integers(0, 2, p[1::9].shape)
        d[2], p[2] = 0, 0
        wd, wrc = oracle_rs(code, d, p)
        assert min(_classes(wrc[:63] == 0, (wd[:63] != d[:63]).any(axis=(1, 2)))) > 0
        for n in (1, 63, 64, N):
            got, st = d[:n].copy(), fe.sentinel((n,))
            assert l.ddn_fec_p25_rs_host(cid, got.ctypes.data, p.ctypes.data, n, st.ctypes.data) == 0
            assert np.array_equal(st, wrc[:n]) and np.array_equal(got, wd[:n]), (code, n)
        d, p, drel, prel = gen_rs_soft(rng, code, 400)
        hard_rc = oracle_rs(code, d, p)[1]
        wd, wrc = oracle_rs_soft_rel(code, d, p, drel, prel)
        first = int(np.flatnonzero((hard_rc != 0) & (wrc == 0))[0])      # hard decode fails, a ranked-erasure retry decodes
        order = [first] + [i for i in range(N) if i != first]
        d, p, drel, prel, wd, wrc, hard_rc = (np.ascontiguousarray(a[order]) for a in (d, p, drel, prel, wd, wrc, hard_rc))
        assert hard_rc[0] != 0 and wrc[0] == 0
        assert min(_classes(wrc[:63] == 0, (wd[:63] != d[:63]).any(axis=(1, 2)))) > 0
        for n in (1, 63, 64, N):
            got, st = d[:n].copy(), fe.sentinel((n,))
            assert l.ddn_fec_p25_rs_soft_host(cid, got.ctypes.data, p.ctypes.data, drel.ctypes.data, prel.ctypes.data, n,
                                              st.ctypes.data) == 0
            assert np.array_equal(st, wrc[:n]) and np.array_equal(got, wd[:n]), (code, n)
    for kind in (0, 1, 2):
        pl, pa, er, ne, _ = _batch(np.random.default_rng(fe.FZ + 110 + kind), kind, N)
        want = [rs28.oracle_rs28(kind, pl[i].astype(np.int32), pa[i].astype(np.int32), er[i, :ne[i]].astype(np.int32)) for i in range(N)]
        wpl, wrc = np.stack([w[0] for w in want]).astype(np.uint8), np.array([w[1] for w in want], np.int32)
        assert min(_classes(wrc[:63] >= 0, (wpl[:63] != pl[:63]).any(axis=1))) > 0
        for n in (1, 63, 64, N):
            got, st = pl[:n].copy(), fe.sentinel((n,), np.int32)
            assert l.ddn_fec_rs28_host(kind, got.ctypes.data, pa.ctypes.data, er.ctypes.data, ne.ctypes.data, n, st.ctypes.data) == 0
            assert np.array_equal(st, wrc[:n]) and np.array_equal(got, wpl[:n]), (kind, n)
    for length in (6, 12):
        rng = np.random.default_rng(fe.FZ + 120 + length)
        d, p = fecgen.gen_golay24(rng, N, length)
        d[1::9], p[1::9] = rng.integers(0, 2, d[1::9].shape), rng.integers(0, 2, p[1::9].shape)
        d[2], p[2] = 0, 0
        d[3, 1] = 2                                                        # an invalid bit value: rc 1, untouched
        wd, wrc, wfx = oracle_golay(d, p)
        assert min(_classes(wrc[:63] == 0, wfx[:63] > 0)) > 0
        for n in (1, 63, 64, N):
            got, st, fx = d[:n].copy(), fe.sentinel((n,)), fe.sentinel((n,), np.int32)
            assert l.ddn_fec_golay24_host(length, got.ctypes.data, p.ctypes.data, n, st.ctypes.data, fx.ctypes.data) == 0
            assert np.array_equal(st, wrc[:n]) and np.array_equal(fx, wfx[:n]) and np.array_equal(got, wd[:n]), (length, n)


def test_soft_golay_and_hamming_hosts_at_their_group_edges(built):
    """k_golay24_soft and k_hamming_10_6_3_soft (256 threads) at n 1 / 255 / 256 / 257: 0 .. 6 flipped bits per word, so clean,
    corrected and rejected words in every batch"""
    from test_oracle_rs import gen_soft_reliab, oracle_golay_soft, oracle_hamming_soft
    l = ddn.lib()
    N = 257
    for length in (6, 12):
        rng = np.random.default_rng(fe.FZ + 130 + length)
        d, p, flips = np.zeros((N, length), np.uint8), np.zeros((N, 12), np.uint8), np.zeros((N, length + 12), bool)
        for i in range(N):
            d12 = np.zeros(12, np.uint8)
            d12[12 - length:] = rng.integers(0, 2, length)
            w = np.concatenate([d12[12 - length:], fecgen.golay24_encode(d12)])
            pos = rng.choice(length + 12, i % 7, replace=False)
            w[pos] ^= 1
            flips[i, pos] = True
            d[i], p[i] = w[:length], w[length:]
        rel = gen_soft_reliab(rng, flips.shape, flips)
        d[20, 0] = 3
        want, wrc, wfx = oracle_golay_soft(d, p, rel)
        assert min(_classes(wrc[:255] == 0, wfx[:255] > 0)) > 0
        for n in (1, 255, 256, N):
            got, st, fx = d[:n].copy(), fe.sentinel((n,)), fe.sentinel((n,), np.int32)
            assert l.ddn_fec_golay24_soft_host(length, got.ctypes.data, p.ctypes.data, rel.ctypes.data, n, st.ctypes.data, fx.ctypes.data) == 0
            assert np.array_equal(st, wrc[:n]) and np.array_equal(fx, wfx[:n]) and np.array_equal(got, want[:n]), (length, n)
    rng = np.random.default_rng(fe.FZ + 140)
    d = rng.integers(0, 2, (N, 6)).astype(np.uint8)
    p = np.stack([d[:, 0] ^ d[:, 1] ^ d[:, 2] ^ d[:, 5], d[:, 0] ^ d[:, 1] ^ d[:, 3] ^ d[:, 5],
                  d[:, 0] ^ d[:, 2] ^ d[:, 3] ^ d[:, 4], d[:, 1] ^ d[:, 2] ^ d[:, 3] ^ d[:, 4]], axis=1)
    bits = np.ascontiguousarray(np.concatenate([d, p], axis=1).astype(np.uint8))
    flips = rng.random(bits.shape) < np.array([0.0, 0.08, 0.3])[np.arange(N) % 3][:, None]
    bits ^= flips.astype(np.uint8)
    rel = gen_soft_reliab(rng, bits.shape, flips)
    bits[10, 3] = 2
    want, wrc = oracle_hamming_soft(bits, rel)
    assert set(wrc[:255].tolist()) == {0, 1, 2}                            # valid, corrected, uncorrectable
    for n in (1, 255, 256, N):
        out, st = fe.sentinel((n, 10)), fe.sentinel((n,))
        assert l.ddn_fec_hamming_10_6_3_soft_host(bits.ctypes.data, rel.ctypes.data, n, out.ctypes.data, st.ctypes.data) == 0
        assert np.array_equal(st, wrc[:n]) and np.array_equal(out, want[:n]), n


def _hex_reliab(llr):
    """reliability of each 6-bit symbol: the least min(|LLR|, 255) of its bits"""
    return np.minimum(np.abs(np.asarray(llr, np.int32)), 255).reshape(-1, 6).min(axis=1)


def _front(items, went_to_retries, n_keep=65):
    """the batch with a section that only a retry decodes in front, then one that fails every retry and one whose ranked list ends
    before max_add; items: (inputs, oracle answer, used_dynamic, failed, list shorter than max_add)"""
    a = next(k for k, it in enumerate(items) if it[2] == 1)
    b = next(k for k, it in enumerate(items) if it[3])
    c = next(k for k, it in enumerate(items) if k not in (a, b) and went_to_retries(it) and it[4])
    out = [items[a], items[b], items[c]] + [it for k, it in enumerate(items) if k not in (a, b, c)]
    return out[:n_keep]


@pytest.mark.parametrize("kind", [0, 1])
def test_xcch_stage_where_the_probe_grid_is_ragged(built, kind):
    """ddn_p25p2_xcch at n 1 / 63 / 65: n * max_add (10 FACCH, 16 SACCH) is no multiple of the probe pass's 64 threads.  Burst 0 fails
    its plain decode and decodes on a retry; every batch of 63 and more also holds a burst that fails every retry and one that goes
    to the retries with a ranked list shorter than max_add (the probe threads past its end)."""
    from test_oracle_p25p2_xcch import N_PL, oracle_xcch
    rng = np.random.default_rng(fe.FZ + 150 + kind)
    min_add, max_add = ((5, 10), (8, 16))[kind]
    items = []
    for i in range(300):
        n_err = int(rng.integers(0, 15))
        b, llr, _ = rs28.make_xcch_burst(rng, kind, n_err, int(rng.integers(0, n_err + 1)), int(rng.integers(0, 8)))
        ec, pl, used = oracle_xcch(kind, b, llr)
        rel = np.concatenate([_hex_reliab(llr[rs28.XCCH_PAYLOAD_POS[kind]]), _hex_reliab(llr[rs28.XCCH_PARITY_POS[kind]])])
        add = min(max(int((rel < 64).sum()), min_add), max_add)
        items.append(((b, llr), (ec, pl), used, ec < 0, add < max_add))
    items = _front(items, lambda it: it[2] == 1 or it[3])
    assert items[0][2] == 1 and items[0][1][0] >= 0
    assert any(it[3] for it in items[:63]) and any((it[2] == 1 or it[3]) and it[4] for it in items[:63])
    bits, llr = np.stack([it[0][0] for it in items]).astype(np.uint8), np.stack([it[0][1] for it in items]).astype(np.int16)
    for n in (1, 63, 65):
        pl, ec, used = fe.sentinel((n, N_PL[kind])), fe.sentinel((n,), np.int32), fe.sentinel((n,))
        assert ddn.lib().ddn_p25p2_xcch_host(kind, bits.ctypes.data, llr.ctypes.data, n, 64, pl.ctypes.data, ec.ctypes.data, used.ctypes.data) == 0
        for i in range(n):
            (wec, wpl), wused = items[i][1], items[i][2]
            assert ec[i] == wec and used[i] == wused and np.array_equal(pl[i], wpl), (kind, n, i, ec[i], wec, used[i], wused)


def test_ess_stage_where_the_probe_grid_is_ragged(built):
    """ddn_p25p2_ess at n 1 / 63 / 65 (28 attempts per section), the same three kinds of section in front as for the bursts"""
    from test_oracle_p25p2_xcch import oracle_ess
    rng = np.random.default_rng(fe.FZ + 160)
    items = []
    for i in range(300):
        n_err = int(rng.integers(0, 26))
        a, b, c, d, _ = rs28.make_ess_case(rng, n_err, int(rng.integers(0, n_err + 1)), int(rng.integers(0, 8)))
        acc, wec, wout = oracle_ess(a, b, c, d)
        plain = rs28.oracle_rs28(0, a.astype(np.int32), c.astype(np.int32), np.zeros(0, np.int32))[1]
        retried = not 0 <= plain < 15                                      # the plain decode failed or located 15 symbols or more
        cnt = min(max(int((np.concatenate([_hex_reliab(b), _hex_reliab(d)]) < 64).sum()), 14), 28)
        items.append(((a, b, c, d), (acc, wec, wout), int(bool(acc) and retried), not acc, cnt < 28))
    items = _front(items, lambda it: it[2] == 1 or it[3])
    assert items[0][2] == 1
    assert any(it[3] for it in items[:63]) and any((it[2] == 1 or it[3]) and it[4] for it in items[:63])
    pl, pll, pa, pal = (np.ascontiguousarray(np.stack([it[0][k] for it in items])) for k in range(4))
    for n in (1, 63, 65):
        out, ec, used = fe.sentinel((n, 96)), fe.sentinel((n,), np.int32), fe.sentinel((n,))
        assert ddn.lib().ddn_p25p2_ess_host(pl.ctypes.data, pll.ctypes.data, pa.ctypes.data, pal.ctypes.data, n, 64, out.ctypes.data,
                                            ec.ctypes.data, used.ctypes.data) == 0
        for i in range(n):
            acc, wec, wout = items[i][1]
            assert (ec[i] >= 0) == bool(acc) and ec[i] == wec and np.array_equal(out[i], wout), (n, i, ec[i], acc, wec)
            assert used[i] == items[i][2], (n, i)


@pytest.mark.parametrize("code", list(RS_ID))
def test_rs_failed_word_with_a_non_binary_byte(built, code):
    """an uncorrectable word with a data byte of 5: the hard entry rewrites the data bits from the uncorrected symbols (the 5 reads
    back as 1), the soft-reliability entry leaves the data as it came - both as the oracle does"""
    from test_oracle_rs import oracle_rs, oracle_rs_soft_rel
    rng = np.random.default_rng(fe.FZ + 170 + RS_ID[code])
    d, p = fecgen.gen_p25_rs(rng, code, 40)
    d[:], p[:] = rng.integers(0, 2, d.shape), rng.integers(0, 2, p.shape)
    d[:, 1, 2] = 5
    drel, prel = np.full(d.shape[:2], 200, np.uint8), np.full(p.shape[:2], 200, np.uint8)
    k = int(np.flatnonzero((oracle_rs(code, d, p)[1] == 1) & (oracle_rs_soft_rel(code, d, p, drel, prel)[1] == 1))[0])
    d, p, drel, prel = (np.ascontiguousarray(a[k:k + 1]) for a in (d, p, drel, prel))      # a random word that both decoders give up on
    wd, wrc = oracle_rs(code, d, p)
    ws, wsrc = oracle_rs_soft_rel(code, d, p, drel, prel)
    assert wrc[0] == 1 and wsrc[0] == 1 and wd[0, 1, 2] == 1 and ws[0, 1, 2] == 5
    got, st = d.copy(), fe.sentinel((1,))
    assert ddn.lib().ddn_fec_p25_rs_host(RS_ID[code], got.ctypes.data, p.ctypes.data, 1, st.ctypes.data) == 0
    assert st[0] == 1 and np.array_equal(got, wd)
    got, st = d.copy(), fe.sentinel((1,))
    assert ddn.lib().ddn_fec_p25_rs_soft_host(RS_ID[code], got.ctypes.data, p.ctypes.data, drel.ctypes.data, prel.ctypes.data, 1,
                                              st.ctypes.data) == 0
    assert st[0] == 1 and np.array_equal(got, ws)


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
        lambda: l.ddn_fec_p25_rs_host(2, p, p, 0, p),
        lambda: l.ddn_fec_p25_rs_soft_host(2, p, p, p, p, 0, p),
        lambda: l.ddn_fec_rs28_host(0, p, p, p, p, 0, p),
        lambda: l.ddn_fec_golay24_host(12, p, p, 0, p, p),
        lambda: l.ddn_fec_golay24_soft_host(12, p, p, p, 0, p, p),
        lambda: l.ddn_fec_hamming_10_6_3_soft_host(p, p, 0, p, p),
    ]
    for k, call in enumerate(calls):
        assert call() == ddn.DDN_OK, (k, l.ddn_last_error())
        assert fe.untouched(a), k
