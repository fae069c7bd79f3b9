"""GPU: the sparse (`wanted`) forms of the FEC decoders - the entries the chains really call - against the oracle, item by item, bit-exact:
wanted items read what the oracle gives for that item alone, unwanted items read what the contract next to each declaration in
csrc/ddn_device.h says (count 0 / zeros / left unwritten / decoded with a wanted neighbour), nothing is written past item n - 1.  Every
output buffer starts as 0xA5 bytes (counts -1) with one guard item behind the batch.  Inputs, patterns and checkers: tests/fec_edge.py;
that the inputs are not easy: tests/test_fec_edge.py."""
import numpy as np
import pytest

import dmr_data  # noqa: F401  (fec_edge's pool restatement)
import fec_edge as fe
import fecgen
import rx4

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def dv(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def dwanted(w):
    """the wanted list on the device, 64 zero bytes behind it (an index past the list reads 'not wanted', not another allocation)"""
    return dv(np.concatenate([np.asarray(w, np.uint8), np.zeros(64, np.uint8)]))


def dsent(shape, dtype=np.uint8, fill=None):
    a = fe.sentinel(shape, dtype)
    if fill is not None:
        a[...] = fill
    return dv(a)


def stream():
    return _torch().cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, (rc, fe.dev().ddn_last_error())


def back(*ts):
    _torch().cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def launch_list(entry, fam, d_rows, d_rel, n, mx, w, N):
    """one sparse launch of a list decoder over the first n of N staged items -> (cand [n + 1][K][stride], cnt [n + 1], backs or None)"""
    L = fe.LAYOUT[fam]
    cand = dsent((n + 1, L["K"], L["stride"]))
    cnt = dsent((n + 1,), np.int32, -1)
    dw = dwanted(w)
    l = fe.dev()
    backs = None
    if fam == "half":
        ok(getattr(l, entry)(d_rows.data_ptr(), n, mx, dw.data_ptr(), cand.data_ptr(), cnt.data_ptr(), stream()))
    elif fam == "mbf":
        ok(l.ddn_fec_p25_mbf34_list_batch(d_rows.data_ptr(), n, mx, dw.data_ptr(), cand.data_ptr(), cnt.data_ptr(), stream()))
    else:
        backs = dsent((n + 1, 49 * 8 * 32))
        ok(l.ddn_dev_r34_list_wanted(d_rows.data_ptr(), d_rel.data_ptr() if d_rel is not None else None, n, mx, dw.data_ptr(),
                                     backs.data_ptr(), cand.data_ptr(), cnt.data_ptr(), stream()))
    out = back(cand, cnt) + ([back(backs)[0]] if backs is not None else [None])
    return out


@pytest.mark.parametrize("fam,weighted,entry", [("half", 0, "ddn_dev_p25_half_rate_list_wanted"),
                                                ("half", 0, "ddn_dev_p25_half_rate_list_wanted_wide"),
                                                ("r34", 0, "ddn_dev_r34_list_wanted"), ("r34", 1, "ddn_dev_r34_list_wanted"),
                                                ("mbf", 0, "ddn_fec_p25_mbf34_list_batch")])
def test_list_decoders_sparse(built, fam, weighted, entry):
    """every batch size around the group, every wanted pattern, max_cand 1 / the full list / 100 (clamped): bytes, metric, order and
    count of the decoded items, the documented read-back of the others, the guard item"""
    G = fe.GROUP[fam] if fam != "mbf" else 4           # (mbf: one item per workgroup; the patterns still come in fours)
    sizes = fe.batch_sizes(G)
    N = sizes[-1]
    rel = None
    if fam == "half":
        rows = fe.half_inputs(N)
    elif fam == "mbf":
        rows = fe.mbf_inputs(N)
    else:
        rows, rel = fe.r34_inputs(N)
        rel = rel if weighted else None
    exps = {mx: [fe.oracle_list(fam, rows[i], mx, rel[i] if rel is not None else None) for i in range(N)] for mx in fe.MAX_CAND[fam]}
    d_rows = dv(rows)
    d_rel = dv(rel) if rel is not None else None
    for n in sizes:
        for p in fe.PATTERNS:
            w = fe.wanted(p, n, G)
            for mx in fe.MAX_CAND[fam]:
                cand, cnt, backs = launch_list(entry, fam, d_rows, d_rel, n, mx, w, N)
                fe.check_list(fam, n, w, cand, cnt, exps[mx], (entry, n, p, mx))
                if backs is not None:              # the scratch of an item nobody wants, and of the guard, stays as it was
                    assert fe.untouched(backs[n]) and all(fe.untouched(backs[i]) for i in range(n) if not w[i]), (n, p, mx)


@pytest.mark.parametrize("entry,cap", [("ddn_dev_p25_half_rate_list_wanted", 1024), ("ddn_dev_p25_half_rate_list_wanted_wide", 16384)])
def test_half_rate_list_past_the_grid_cap(built, entry, cap):
    """n = 4 cap + 5: workgroups 0 and 1 take a second group (the last one ragged) after their first.  'split': decode then skip, and skip
    then decode; 'both': a second decode over the LDS arrays of the first - stale LDS shows as a decoded item that is not the oracle's"""
    n = 4 * cap + 5
    llr = fe.half_inputs(n, seed=cap)
    d_rows = dv(llr)
    for name, w in fe.wrap_layouts(n, cap).items():
        cand, cnt, _ = launch_list(entry, "half", d_rows, None, n, 8, w, n)
        dm = fe.decoded_mask("half", w)
        assert dm.sum() <= 600
        for i in np.nonzero(dm)[0]:
            fe.check_list_item("half", cand[i], cnt[i], fe.oracle_list("half", llr[i], 8), True, (entry, name, int(i)))
        assert (cnt[:n][~dm] == 0).all(), (entry, name)
        assert fe.untouched(cand[:n][~dm]) and fe.untouched(cand[n]) and cnt[n] == -1, (entry, name)


@pytest.mark.parametrize("soft", [0, 1])
@pytest.mark.parametrize("steps,nbits,div", [(96, 92, 2), (36, 32, 1), (148, 144, 1), (201, 197, 1)])
def test_k5_nxdn_wanted(built, steps, nbits, div, soft):
    """the callers' shapes: FACCH (two rows per slot, wanted_div = 2), SACCH, the M17 stream and BERT frames.  Wanted rows are the
    oracle's (with the metrics carried in and out where given); an unwanted row reads zeros in an empty group of 16 and its decode beside
    a wanted row, and its metrics and the bytes behind (n_bits + 7) / 8 stay as they were"""
    slots = fe.batch_sizes(16 // div)
    R = slots[-1] * div
    sym, rel, m0 = fe.nxdn_inputs(R, steps)
    rel = rel if soft else None
    nby = (nbits + 7) // 8
    stride = nby + 2
    exp = {False: fecgen.oracle_nxdn(sym, rel, steps, nbits), True: fecgen.oracle_nxdn(sym, rel, steps, nbits, metrics=m0)}
    d_sym, d_rel = dv(sym), (dv(rel) if soft else None)
    l = fe.dev()
    for S in slots:
        n = S * div
        for p in fe.PATTERNS:
            w = fe.wanted(p, S, 16 // div)
            rows_wanted = np.repeat(w, div).astype(bool)
            for with_m in (False, True):
                out, dw = dsent((n + 1, stride)), dwanted(w)
                dm = None
                if with_m:
                    mh = fe.sentinel((n + 1, 16), np.uint16)
                    mh[:n] = m0[:n]
                    dm = dv(mh)
                ok(l.ddn_dev_k5_nxdn_wanted(d_sym.data_ptr(), d_rel.data_ptr() if soft else None, n, steps, nbits,
                                            dm.data_ptr() if with_m else None, out.data_ptr(), stride, dw.data_ptr(), div, stream()))
                got = back(out)[0]
                where = (steps, div, soft, n, p, with_m)
                fe.check_rows(n, rows_wanted, 16, got, nby, exp[with_m][0], "zero", where)
                if with_m:
                    gm = back(dm)[0]
                    want_m = np.where(rows_wanted[:, None], exp[True][1][:n], m0[:n])
                    assert np.array_equal(gm[:n], want_m), where
                    assert fe.untouched(gm[n]), where


@pytest.mark.parametrize("in_len,punct", fe.M17_SHAPES, ids=["200", "360", "420"])
def test_k5_m17_wanted(built, in_len, punct):
    """ddn_fec_viterbi_k5_batch_wanted at the three shapes of ddn_api_m17.cpp: a code word in a group of 16 with no wanted one keeps
    whatever its row and cost held; beside a wanted one it is decoded"""
    sizes = fe.batch_sizes(16)
    N = sizes[-1]
    soft = fecgen.gen_m17(np.random.default_rng(fe.FZ + 61 + in_len), N, in_len, sigma=20000.0)
    wo, wc, need = fecgen.oracle_m17(soft, punct)
    stride = 16 if in_len == 200 else 32
    assert need <= stride
    d_soft = dv(soft)
    l = fe.dev()
    for n in sizes:
        for p in fe.PATTERNS:
            w = fe.wanted(p, n, 16)
            out, cost, dw = dsent((n + 1, stride)), dsent((n + 1,), np.uint32), dwanted(w)
            ok(l.ddn_fec_viterbi_k5_batch_wanted(d_soft.data_ptr(), n, in_len, punct.ctypes.data if punct is not None else None,
                                                 len(punct) if punct is not None else 0, out.data_ptr(), stride, cost.data_ptr(),
                                                 dw.data_ptr(), stream()))
            go, gc = back(out, cost)
            dec = fe.check_rows(n, w, 16, go, need, wo, "kept", (in_len, n, p), extra="zero")
            for i in range(n):
                assert (gc[i] == wc[i]) if dec[i] else fe.untouched(gc[i:i + 1]), (in_len, n, p, i)
            assert fe.untouched(gc[n:])


def test_trellis_greedy_wanted(built):
    """the NXDN SACCH retry (72 input bits a row, 32 out): an unwanted row reads zeros, row by row; the two bytes behind a row stay"""
    sizes = fe.batch_sizes(64)
    N = sizes[-1]
    src = fe.greedy_inputs(N)
    exp = rx4.oracle_trellis_decode(src, 32)
    d_src = dv(src)
    for n in sizes:
        for p in fe.PATTERNS:
            w = fe.wanted(p, n, 64)
            out, dw = dsent((n + 1, 34)), dwanted(w)
            ok(fe.dev().ddn_dev_trellis_greedy_wanted(d_src.data_ptr(), src.shape[1], n, 32, out.data_ptr(), 34, dw.data_ptr(), stream()))
            fe.check_rows(n, w, 1, back(out)[0], 32, exp, "zero", (n, p))


def test_dmr_r34_pick_item_by_item(built):
    """k_dmr_r34_pick over the product's own hard, soft and list decodes: the pool (metric, 18 bytes, CRC9 flag, DBSN, in pool order),
    its length and the two picks against dmr_data.pool_of() / pick_unconfirmed() / pick_confirmed(); list_n 0 and 32; unwanted bursts
    read the kernel's zero fill over an unwritten pool"""
    N = 200
    td, rel, kinds = fe.pick_inputs(N)
    d_td, d_rel = dv(td), dv(rel)
    hard, soft = dsent((N, 18)), dsent((N, 18))
    lst, lstn = dsent((N, 32, 24)), dsent((N,), np.int32, -1)
    l = fe.dev()
    ok(l.ddn_fec_r34_batch(d_td.data_ptr(), None, N, hard.data_ptr(), None))
    ok(l.ddn_fec_r34_batch(d_td.data_ptr(), d_rel.data_ptr(), N, soft.data_ptr(), None))
    ok(l.ddn_fec_r34_list_batch(d_td.data_ptr(), d_rel.data_ptr(), N, 32, lst.data_ptr(), lstn.data_ptr(), None))
    h_hard, h_soft, h_lst, h_n = back(hard, soft, lst, lstn)
    assert (h_n == 32).all()
    h_n = h_n.copy()
    h_n[[i for i in range(N) if kinds[i] == "clean"][::2]] = 0        # list_n = 0: with hard = soft a pool of one
    h_n[5::31] = 0
    lstn = dv(h_n)
    exp = [fe.expected_pick(td[i], rel[i], h_hard[i], h_soft[i], h_lst[i], h_n[i]) for i in range(N)]
    assert min(len(e[0]) for e in exp) == 1 and max(len(e[0]) for e in exp) >= 33
    for n in (1, 63, 64, 65, 200):
        for p in fe.PATTERNS:
            w = fe.wanted(p, n, 64)
            pool, pool_n = dsent((n + 1, 34, 24)), dsent((n + 1,), np.int32, -1)
            unconf, conf, crc, dw = dsent((n + 1, 18)), dsent((n + 1, 18)), dsent((n + 1,)), dwanted(w)
            ok(l.ddn_dev_dmr_r34_pick(d_td.data_ptr(), d_rel.data_ptr(), dw.data_ptr(), hard.data_ptr(), soft.data_ptr(),
                                      lst.data_ptr(), lstn.data_ptr(), n, pool.data_ptr(), pool_n.data_ptr(), unconf.data_ptr(),
                                      conf.data_ptr(), crc.data_ptr(), stream()))
            g_pool, g_n, g_u, g_c, g_crc = back(pool, pool_n, unconf, conf, crc)
            for i in range(n):
                where = (n, p, i, kinds[i])
                if w[i]:
                    p24, u, c, ok9 = exp[i]
                    assert g_n[i] == len(p24), where
                    assert np.array_equal(g_pool[i, :len(p24)], p24), where
                    assert fe.untouched(g_pool[i, len(p24):]), where
                    assert np.array_equal(g_u[i], u) and np.array_equal(g_c[i], c) and g_crc[i] == ok9, where
                else:
                    assert g_n[i] == 0 and g_crc[i] == 0 and not g_u[i].any() and not g_c[i].any(), where
                    assert fe.untouched(g_pool[i]), where
            assert g_n[n] == -1 and fe.untouched(g_pool[n]) and fe.untouched(g_u[n]) and fe.untouched(g_c[n]) and fe.untouched(g_crc[n:])
