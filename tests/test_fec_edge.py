"""CPU: the helpers of the FEC decoders' edge tests (tests/fec_edge.py) and the floors of their inputs, with the oracle alone - so that
no device test passes by being easy.

Floors of the list decoders.  Among the wanted items of a case there should be one with fewer candidates than max_cand, one with the
full max_cand, one with a duplicate removed and one with two candidates of equal metric.  What the decoders' structure allows, read from
the oracle (oracle/ddn_oracle_fec.c) and asserted below for every item:
  * after the third step every state of the three trellises holds a full survivor list, so the final survivors are always 32 (half: 4
    states x 8), 32 (r34: state 0's list) and 64 (mbf: 8 x 8), and the paths of one final state are distinct in the bytes.  The count is
    therefore min(max_cand, K) for EVERY input: "fewer than max_cand" happens exactly where max_cand is above K (the 100 the kernels
    clamp), "the full max_cand" at 1 and K - both are cases of every family, on every wanted item;
  * a duplicate is removed where two final states share their first 48 states (half, mbf: the bytes leave the 49th out) - the oracle
    counts them (orc_list_last_stats); the r34 list is never de-duplicated (all 32 candidates end in state 0 and differ), which the test
    asserts instead;
  * ties need equal metrics: the all-zero and saturated rows, and the unweighted r34 costs.
The tie and duplicate floors are asserted on the wanted items of every pattern that wants more than three items, and on the union."""
import numpy as np
import pytest

import dmr_data
import fec_edge as fe
import fecgen


def test_wanted_patterns_are_what_they_say():
    for G in (1, 4, 8, 16, 64):
        for n in fe.batch_sizes(G):
            ng = (n + G - 1) // G
            pats = {p: fe.wanted(p, n, G) for p in fe.PATTERNS}
            assert all(len(w) == n and w.dtype == np.uint8 and set(np.unique(w)) <= {0, 1} for w in pats.values())
            assert not pats["all0"].any() and pats["all1"].all()
            assert pats["first"].sum() == 1 and pats["first"][0] == 1
            assert pats["last"].sum() == 1 and pats["last"][n - 1] == 1
            assert np.array_equal(np.nonzero(pats["alternating"])[0], np.arange(0, n, 2))
            per = [int(pats["one_per_group"][g * G:(g + 1) * G].sum()) for g in range(ng)]
            assert per == [1] * ng
            og = [int(pats["one_group"][g * G:(g + 1) * G].sum()) for g in range(ng)]
            assert sorted(og)[:-1] == [0] * (ng - 1) and max(og) == len(pats["one_group"][og.index(max(og)) * G:][:G])
            if ng >= 3:
                assert og[0] == 0 and og[1] == G and og[2] == 0
            assert 1 <= pats["random5"].sum() <= max(1, n // 4)
        assert fe.batch_sizes(G)[-1] == 3 * G + 1 and (3 * G + 1) % G == (1 % G)         # a ragged last group
    assert fe.batch_sizes(4) == [1, 3, 4, 5, 13] and fe.batch_sizes(16) == [1, 15, 16, 17, 49]


def test_group_masks():
    w = np.array([0, 0, 0, 0, 0, 1, 0, 0, 0], np.uint8)
    assert fe.group_has_wanted(w, 4).tolist() == [False] * 4 + [True] * 4 + [False]
    assert fe.decoded_mask("half", w).tolist() == fe.group_has_wanted(w, 4).tolist()
    assert fe.decoded_mask("r34", w).tolist() == w.astype(bool).tolist()
    assert fe.decoded_mask("mbf", w).tolist() == w.astype(bool).tolist()


@pytest.mark.parametrize("cap", [1024, 16384])
def test_wrap_layouts_put_both_orders_on_the_wrapping_workgroups(cap):
    n = 4 * cap + 5
    lay = fe.wrap_layouts(n, cap)
    assert (n + 3) // 4 == cap + 2                      # two groups past the cap: the second groups of workgroups 0 and 1
    s = fe.group_has_wanted(lay["split"], 4)
    assert s[0] and not s[4 * cap] and not s[4] and s[4 * cap + 4]          # wg 0: first decoded, second skipped; wg 1 the other way
    b = fe.group_has_wanted(lay["both"], 4)
    assert b[0] and b[4 * cap] and b[4] and b[4 * cap + 4]
    for w in lay.values():
        assert 100 <= w.sum() <= 300 and len(w) == n
        assert not w[n - 5:n - 1].all()                  # the last full group stays mixed or empty: a per-item answer is checked there


def _list_case(fam, weighted):
    G = fe.GROUP[fam]
    n = 3 * G + 1 if fam != "mbf" else 13
    if fam == "half":
        rows, rel = fe.half_inputs(n), None
    elif fam == "mbf":
        rows, rel = fe.mbf_inputs(n), None
    else:
        rows, rel = fe.r34_inputs(n)
        rel = rel if weighted else None
    return G, n, rows, rel


@pytest.mark.parametrize("fam,weighted", [("half", 0), ("mbf", 0), ("r34", 0), ("r34", 1)])
def test_list_decoder_inputs_meet_the_floors(fam, weighted):
    G, n, rows, rel = _list_case(fam, weighted)
    K = fe.LAYOUT[fam]["K"]
    ties, dups = np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        r = rel[i] if rel is not None else None
        for mx in fe.MAX_CAND[fam]:
            no, by, me = fe.oracle_list(fam, rows[i], mx, r)
            assert no == min(mx, K), (fam, i, mx, no)                            # (the structural fact of the docstring)
            assert len({bytes(b) for b in by}) == no
            assert np.all(np.diff(me.astype(np.int64)) >= 0)
            if mx == K:
                ties[i] = bool((np.diff(me.astype(np.int64)) == 0).any())
                if fam != "r34":
                    paths, dropped = fe.list_stats()
                    assert paths == (32 if fam == "half" else 64)
                    dups[i] = dropped > 0
    assert 100 > K and 1 < K                                                     # fewer than max_cand at 100, the full list at 1 and K
    assert ties[0] and ties[n - 1]                                               # the all-zero rows
    union = np.zeros(n, bool)
    for p in fe.PATTERNS:
        w = fe.wanted(p, n, G).astype(bool)
        union |= w
        if w.sum() > 3:
            assert (ties & w).any(), (fam, p)
            assert fam == "r34" or (dups & w).any(), (fam, p)
    assert (ties & union).any()
    assert fam == "r34" or ((dups & union).any())


def test_wrapping_batches_want_items_with_ties_and_duplicates():
    """the two capped-grid batches: the wanted items of the wrapping groups include the all-zero rows at both ends (ties, duplicates)"""
    for cap in (1024,):
        n = 4 * cap + 5
        llr = fe.half_inputs(n, seed=cap)
        for w in fe.wrap_layouts(n, cap).values():
            assert w[0] and w[n - 1]
            for i in (0, n - 1):
                no, by, me = fe.oracle_list("half", llr[i], 8)
                assert no == 8 and (np.diff(me.astype(np.int64)) == 0).any() and fe.list_stats()[1] > 0


def _oracle_decodes(td, rel):
    import ctypes as C
    o = fecgen.bind_oracle_fec()
    o.orc_r34_decode_list.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    n = len(td)
    hard, soft = fecgen.oracle_r34(td), fecgen.oracle_r34(td, rel)
    cands = np.zeros((n, 32, 24), np.uint8)
    cnt = np.zeros(n, np.int32)
    for i in range(n):
        no, by, me = fe.oracle_list("r34", td[i], 32, rel[i])
        cands[i, :no, 4:22] = by
        cands[i, :no, 0:4] = me.astype(np.int32).view(np.uint8).reshape(no, 4)
        cnt[i] = no
    return hard, soft, cands, cnt


def test_pick_inputs_meet_the_floors():
    n = 70
    td, rel, kinds = fe.pick_inputs(n)
    assert set(kinds) == set(fe.PICK_KINDS)
    hard, soft, cands, cnt = _oracle_decodes(td, rel)
    assert (cnt == 32).all()
    pool_one = crc_beats = hs_differ = full_pool = no_crc = 0
    for i in range(n):
        p24, u, c, crc = fe.expected_pick(td[i], rel[i], hard[i], soft[i], cands[i], cnt[i])
        pool, ru, rc, rcrc = dmr_data.r34_pool(td[i], rel[i])                    # the helper restates dmr_data.r34_pool()
        assert len(pool) == len(p24) and np.array_equal(u, ru) and np.array_equal(c, rc) and crc == rcrc
        for k, (b, metric, ok, dbsn) in enumerate(pool):
            assert np.array_equal(p24[k, 4:22], b) and int(p24[k, 0:4].copy().view(np.int32)[0]) == metric
            assert p24[k, 22] == ok and p24[k, 23] == dbsn
        metrics = p24[:, 0:4].copy().view(np.int32).reshape(-1)
        hs_differ += int(not np.array_equal(hard[i], soft[i]))
        full_pool += int(len(p24) >= 33)
        no_crc += int(not crc)
        if kinds[i] == "crc_second":
            assert crc and np.array_equal(hard[i], soft[i])
            k = [j for j in range(len(p24)) if np.array_equal(p24[j, 4:22], c)][0]
            assert p24[k, 22] == 1 and k >= 1 and metrics[k] > metrics.min()   # a dearer list candidate with a good CRC9 wins
            assert not np.array_equal(c, u)
            crc_beats += 1
        if kinds[i] == "clean":
            p1 = fe.expected_pick(td[i], rel[i], hard[i], soft[i], cands[i], 0)      # list_n = 0 and hard = soft: a pool of one
            assert np.array_equal(hard[i], soft[i]) and len(p1[0]) == 1
            pool_one += 1
    assert pool_one >= 5 and crc_beats >= 5 and hs_differ >= 5 and full_pool >= 1 and no_crc >= 5


def test_nxdn_lds_need_is_the_launchers():
    assert fe.nxdn_lds_bytes(1024, False) == 65584 and fe.nxdn_lds_bytes(1024, True) == 98384
    assert fe.nxdn_lds_bytes(1023, False) <= 65536 < fe.nxdn_lds_bytes(1024, False)
    assert fe.nxdn_lds_bytes(681, True) <= 65536 < fe.nxdn_lds_bytes(682, True)


def test_m17_oracle_takes_the_edge_patterns():
    """fecgen.oracle_m17 walks any pattern like viterbi_decode_punctured: the depunctured length of the edge cases, and an erased soft bit
    costs the decoder nothing in the reported cost (0x7FFF per erasure is taken off again)"""
    rng = np.random.default_rng(fe.FZ + 5)
    for in_len, punct, u_len in fe.K5_CASES:
        soft = fecgen.gen_m17(rng, 2, in_len, sigma=20000.0)
        out, cost, stride = fecgen.oracle_m17(soft, punct)
        assert stride == (u_len // 2 + 3) // 8 + 1, (in_len, u_len, stride)
        assert u_len <= 488 and fe.depunctured_len(in_len, punct) == u_len
    for in_len, punct, u_len in fe.K5_TOO_LONG:
        assert fe.depunctured_len(in_len, punct) == u_len > 488
    assert fe.K5_CASES[-1][1][0] == 0 and len(fe.K5_CASES[-1][1]) == 64
