"""Inputs, oracle wrappers and per-item checkers of the FEC decoders' edge tests (tests/test_fec_edge.py on the CPU,
tests/test_fec_sparse_gpu.py and tests/test_fec_limits_gpu.py on the device).  The chains do not run the decoders' dense public forms
but internal sparse ones that take a `wanted` byte list; what an unwanted item reads back differs from family to family and is written
next to each declaration in csrc/ddn_device.h.  This module restates those contracts as checkers over sentinel-filled buffers, so that
"left unwritten", "zeroed" and "decoded anyway" can be told apart.  Pure numpy + the CPU oracle; nothing here touches a device
(dev() only binds prototypes).

Group sizes (read from the launchers in ddn_trellis.hip / ddn_fec3.hip):
  half   k_p25_half_rate_list<4, 64>   4 code words per group, grid capped at 1024 (16384: _wide) workgroups that stride over the groups
  r34    k_r34_list                    8 per workgroup (one wavefront), per-item skip inside a live group
  k5     k_k5_nxdn / k_k5_m17          16 per workgroup, group-level skip only
  lane   k_trellis_greedy / k_dmr_r34_pick   one item per lane, workgroups of 64, per-item skip
  mbf    k_p25_mbf34_list              one item per workgroup, min(n, 65536) workgroups that stride over the items"""
import ctypes as C
import os

import numpy as np

import dmr_data
import fecgen
import orc
import p25gen

FZ = 7919 * int(os.environ.get("DDN_FUZZ_BASE", "0"))
SENT = 0xA5
VP = C.c_void_p
GROUP = dict(half=4, r34=8, k5=16, lane=64, mbf=1)
PATTERNS = ("all0", "all1", "first", "last", "alternating", "one_per_group", "one_group", "random5")
MAX_CAND = dict(half=(1, 8, 100), r34=(1, 32, 100), mbf=(1, 8, 100))     # 100: the kernels clamp to the list length

# candidate layouts: entries of `stride` bytes, the payload at b0, the metric (32 bits, little endian) at m0; zero_tail = the entries
# [count .. K) of a decoded item are zero (the dense tests require it of half and r34; mbf leaves them unwritten)
LAYOUT = dict(half=dict(K=8, stride=16, b0=0, nb=12, m0=12, mtype=np.uint32, zero_tail=True),
              r34=dict(K=32, stride=24, b0=4, nb=18, m0=0, mtype=np.int32, zero_tail=True),
              mbf=dict(K=8, stride=24, b0=0, nb=18, m0=20, mtype=np.uint32, zero_tail=False))


def batch_sizes(G):
    """n around a group of G: 1, G - 1, G, G + 1, 3 G + 1"""
    return sorted({1, max(1, G - 1), G, G + 1, 3 * G + 1})


def wanted(name, n, G, seed=0):
    """the wanted list `name` over n items in groups of G"""
    w = np.zeros(n, np.uint8)
    ng = (n + G - 1) // G
    if name == "all0":
        pass
    elif name == "all1":
        w[:] = 1
    elif name == "first":
        w[0] = 1
    elif name == "last":
        w[n - 1] = 1
    elif name == "alternating":
        w[0::2] = 1
    elif name == "one_per_group":            # a different place in every group; the ragged last group gets its last item
        for g in range(ng):
            w[min(g * G + g % G, n - 1)] = 1
    elif name == "one_group":                # a whole group between empty ones (the last group where there are fewer than three)
        g = 1 if ng >= 3 else ng - 1
        w[g * G:(g + 1) * G] = 1
    elif name == "random5":
        rng = np.random.default_rng(FZ + 1000 * seed + n)
        w[:] = rng.random(n) < 0.05
        if not w.any():
            w[int(rng.integers(0, n))] = 1
    else:
        raise KeyError(name)
    return w


def group_has_wanted(w, G):
    """per item: whether any item of its group of G is wanted"""
    w = np.asarray(w, bool)
    n = len(w)
    pad = np.zeros((n + G - 1) // G * G, bool)
    pad[:n] = w
    return np.repeat(pad.reshape(-1, G).any(axis=1), G)[:n]


def decoded_mask(fam, w):
    """which items the family's sparse kernel decodes: half decodes a whole group of 4 as soon as one of it is wanted"""
    return group_has_wanted(w, 4) if fam == "half" else np.asarray(w, bool)


def wrap_layouts(n, cap):
    """the two wanted lists of a half-rate batch that runs past its grid cap of `cap` workgroups (n = 4 cap + 5: groups cap and cap + 1
    are the second groups of workgroups 0 and 1, the last of them ragged).  'split': workgroup 0 decodes its first group and skips its
    second, workgroup 1 the other way round; 'both': both decode both (a second decode over the first one's LDS).  A few more wanted
    items in between, at most 300 in all."""
    assert n == 4 * cap + 5
    rng = np.random.default_rng(FZ + cap)
    out = {}
    for name in ("split", "both"):
        w = np.zeros(n, np.uint8)
        w[rng.choice(np.arange(8, 4 * cap), 120, replace=False)] = 1
        w[0:4] = 1                           # group 0 (workgroup 0, first)
        w[4:8] = 0                           # group 1 (workgroup 1, first)
        w[4 * cap:4 * cap + 4] = 0           # group cap (workgroup 0, second)
        w[4 * cap + 4] = 1                   # group cap + 1 (workgroup 1, second; one item)
        if name == "both":
            w[5] = 1
            w[4 * cap + 2] = 1
        assert w.sum() <= 300
        out[name] = w
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _special(x, zero, hi, lo, step):
    """rows that put every tie-break in play: all-zero rows at both ends, a saturated row, a row saturated the other way at every
    second place, and every third row from the fifth on in coarse steps (few distinct costs, so many paths of equal metric - in every
    group of every family)"""
    n = len(x)
    for i in range(4, n, 3):
        x[i] = (x[i].astype(np.int64) // step) * step
    x[0] = zero
    x[n - 1] = zero
    if n > 2:
        x[1] = hi
    if n > 3:
        x[2, ::2] = lo
    return x


def half_inputs(n, seed=0):
    llr, _ = fecgen.gen_p25_half_rate(np.random.default_rng(FZ + 31 + seed), n, sigma=500.0, random_frac=0.3)
    return _special(llr, 0, 32767, -32768, 1024)


def mbf_inputs(n, seed=0):
    """rate 3/4 LLR blocks: valid code words at a few strengths, weak and flipped places, noise (the families of
    tests/test_oracle_mbf34.py), all-zero and saturated rows"""
    rng = np.random.default_rng(FZ + 37 + seed)
    x = np.zeros((n, 196), np.int16)
    for i in range(n):
        dib = p25gen.encode_three_quarter_rate(rng.integers(0, 256, 18).astype(np.uint8))
        bits = np.stack([(dib >> 1) & 1, dib & 1], axis=1).reshape(-1).astype(np.int64)
        kind = i % 4
        if kind == 0:
            v = (2 * bits - 1) * 200
            weak = rng.choice(196, 12, replace=False)
            v[weak] = (2 * bits[weak] - 1) * rng.integers(1, 12, 12)
        elif kind == 1:
            v = (2 * bits - 1) * 60 + rng.integers(-20, 21, 196)
            f = rng.choice(196, 6, replace=False)
            v[f] = -v[f]
        elif kind == 2:
            v = (2 * bits - 1) * rng.integers(1, 4) + rng.integers(-3, 4, 196)       # many equal metrics
        else:
            v = rng.integers(-300, 301, 196)
        x[i] = v
    return _special(x, 0, 32767, -32768, 100)


def r34_inputs(n, seed=0):
    d, rel, _ = fecgen.gen_r34(np.random.default_rng(FZ + 41 + seed), n, p_err=0.06, random_frac=0.3)
    return d, _special(rel, 0, 255, 0, 128)


def nxdn_inputs(n, n_steps, seed=0):
    rng = np.random.default_rng(FZ + 43 + seed + n_steps)
    sym, rel = fecgen.gen_nxdn(rng, n, n_steps, p_err=0.1)
    m0 = rng.integers(0, 65536, (n, 16)).astype(np.uint16)
    return sym, rel, m0


M17_PUNCT4 = np.array([1, 1, 1, 1], np.uint8)      # the 4-entry pattern of ddn_api_m17.cpp (DSD_YSF_PUNCTURE_NONE: keeps every soft bit)
M17_SHAPES = ((200, M17_PUNCT4), (360, M17_PUNCT4), (420, None))


def depunctured_len(in_len, punct):
    """the walk of viterbi_decode_punctured: how many soft bits the decoder sees for in_len received ones"""
    if punct is None:
        return in_len
    i = u = 0
    while i < in_len:
        i += int(punct[u % len(punct)] != 0)
        u += 1
    return u


_P64 = np.random.default_rng(64).integers(0, 2, 64).astype(np.uint8)
_P64[0], _P64[63] = 0, 1
# (in_len, pattern, the depunctured length worked out by hand; None = by depunctured_len): p_len 1; a pattern that starts with 0; an
# in_len that ends inside a period (odd in_len); an odd unpunctured length; an odd depunctured length; exactly 488 through a pattern
# that starts with 0; p_len 64
K5_CASES = [(96, np.array([1], np.uint8), 96), (100, np.array([0, 1, 1], np.uint8), 150), (101, np.array([1, 1, 0, 1], np.uint8), 134),
            (97, None, 97), (98, np.array([1, 0, 1], np.uint8), 147), (244, np.array([0, 1], np.uint8), 488), (150, _P64, None)]
K5_CASES = [(a, p, u if u is not None else depunctured_len(a, p)) for a, p, u in K5_CASES]
# refused with DDN_ERANGE: 489 and 490 depunctured soft bits, one and two above the decoder's 244-step history
K5_TOO_LONG = [(245, np.array([1, 0], np.uint8), 489), (245, np.array([0, 1], np.uint8), 490)]


def greedy_inputs(n, result_len=32, seed=0):
    """rows of 2 result_len + 8 bits for trellis_decode: a third valid code words with a few flips, the rest random"""
    rng = np.random.default_rng(FZ + 47 + seed)
    src = rng.integers(0, 2, (n, 2 * result_len + 8), dtype=np.uint8)
    for i in range(0, n, 3):
        bits = rng.integers(0, 2, (1, result_len + 4)).astype(np.int64)
        row = fecgen.conv_k5_encode(bits)[0]
        f = rng.choice(len(row), int(rng.integers(0, 4)), replace=False)
        row[f] ^= 1
        src[i] = row
    return src


def dmr_confirmed_block(dbsn, payload16):
    """DBSN(7) | CRC9(9) | 16 bytes as a DMR rate 3/4 confirmed data block carries them: the CRC9 runs over the payload, then the DBSN,
    and is stored inverted (what dmr_data.pool_of() checks)"""
    bits = list(np.unpackbits(np.asarray(payload16, np.uint8))) + [(dbsn >> (6 - i)) & 1 for i in range(7)]
    c = p25gen.crc9(bits) ^ 0x1FF
    return np.array([((dbsn & 0x7F) << 1) | (c >> 8), c & 0xFF] + [int(v) for v in payload16], np.uint8)


PICK_KINDS = ("clean", "few", "many", "random", "rel0", "rel255", "crc_second")


def pick_inputs(n, seed=0):
    """DMR rate 3/4 bursts for the candidate pool, kind k = i % 7: clean code words (hard = soft), a few and many dibit errors with low
    reliability where the error is, random dibits, reliabilities all 0 and all 255, and 'crc_second': a block A with a good CRC9 sent as
    its neighbour B (one tribit changed: CRC9 bad, three payload bits away) with the two dibit pairs where they differ marked unreliable -
    both plain decodes give B at cost 0, the list holds A a little dearer, and the confirmed pick must take A.
    -> (td98 [n][98], rel98 [n][98], kinds [n])"""
    rng = np.random.default_rng(FZ + 53 + seed)
    td = np.zeros((n, 98), np.uint8)
    rel = np.zeros((n, 98), np.uint8)
    il = fecgen.tables()["il"].astype(np.int64)
    kinds = []
    for i in range(n):
        kind = PICK_KINDS[i % len(PICK_KINDS)]
        kinds.append(kind)
        a = dmr_confirmed_block(int(rng.integers(0, 128)), rng.integers(0, 256, 16))
        d = p25gen.encode_three_quarter_rate(a)
        r = rng.integers(100, 256, 98)
        if kind in ("few", "many"):
            f = rng.choice(98, 3 if kind == "few" else 20, replace=False)
            d[f] = rng.integers(0, 4, len(f))
            r[f] = rng.integers(0, 80, len(f))
        elif kind == "random":
            d = rng.integers(0, 4, 98)
            r = rng.integers(0, 256, 98)
        elif kind == "rel0":
            d[rng.choice(98, 4, replace=False)] ^= 1
            r[:] = 0
        elif kind == "rel255":
            d[rng.choice(98, 4, replace=False)] ^= 1
            r[:] = 255
        elif kind == "crc_second":
            t = int(rng.integers(2, 46))
            b = a.copy()
            bits = np.unpackbits(b)
            bits[3 * t + int(rng.integers(0, 3))] ^= 1
            b = np.packbits(bits)
            d = p25gen.encode_three_quarter_rate(b)
            r[:] = 255
            for pair in (t, t + 1):          # the two transitions that see tribit t: de-interleaved dibits 2 pair, 2 pair + 1
                for k in (2 * pair, 2 * pair + 1):
                    r[np.nonzero(il == k)[0][0]] = 1
        td[i] = d
        rel[i] = r
    return td, rel, kinds


# ---- oracle wrappers: one item at a time ----------------------------------------------------------------------------------------------
def _orc():
    o = orc.oracle()
    o.orc_p25_12_soft_llr_list.argtypes = [VP, VP, VP, C.c_int]
    o.orc_r34_decode_list.argtypes = [VP, VP, C.c_int, VP, VP]
    o.orc_p25_mbf34_list.argtypes = [VP, C.c_int, VP, VP]
    o.orc_list_last_stats.argtypes = [VP]
    o.orc_list_last_stats.restype = None
    return o


def list_stats():
    """(survivors traced, dropped as duplicates) at the merge of the last half / mbf oracle call"""
    s = np.zeros(2, np.int32)
    _orc().orc_list_last_stats(s.ctypes.data)
    return int(s[0]), int(s[1])


def oracle_list(fam, row, mx, rel=None):
    """the oracle's candidates of one item -> (count, bytes [count][nb], metrics [count])"""
    o = _orc()
    L = LAYOUT[fam]
    by = np.zeros((L["K"], L["nb"]), np.uint8)
    me = np.zeros(L["K"], L["mtype"])
    row = np.ascontiguousarray(row)
    if fam == "half":
        no = o.orc_p25_12_soft_llr_list(row.ctypes.data, by.ctypes.data, me.ctypes.data, mx)
    elif fam == "mbf":
        no = o.orc_p25_mbf34_list(row.ctypes.data, mx, by.ctypes.data, me.ctypes.data)
    else:
        rel = None if rel is None else np.ascontiguousarray(rel)
        no = o.orc_r34_decode_list(row.ctypes.data, rel.ctypes.data if rel is not None else None, mx, me.ctypes.data, by.ctypes.data)
    return no, by[:no].copy(), me[:no].copy()


# ---- checkers over sentinel-filled buffers ---------------------------------------------------------------------------------------------
def sentinel(shape, dtype=np.uint8):
    """an output buffer as the tests hand it to a kernel: 0xA5 bytes (int32 counts read -1 where a test fills them with -1 instead)"""
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = SENT
    return a


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == SENT).all())


def check_list_item(fam, cand_i, cnt_i, exp, decoded, where=None):
    """one item of a list decoder: cand_i [K][stride] u8, cnt_i its count, exp = oracle_list() of the item (None for an item the kernel
    must not decode).  decoded: count, bytes, metrics and order are the oracle's, pad bytes zero, the tail zero (half, r34) or unwritten
    (mbf).  not decoded: count 0 over unwritten candidates - never a count over bytes that are not the oracle's."""
    L = LAYOUT[fam]
    if not decoded:
        assert cnt_i == 0 and untouched(cand_i), (fam, where, int(cnt_i))
        return
    no, ob, om = exp
    assert cnt_i == no, (fam, where, int(cnt_i), no)
    got = cand_i[:no]
    assert np.array_equal(got[:, L["b0"]:L["b0"] + L["nb"]], ob), (fam, where)
    gm = np.ascontiguousarray(got[:, L["m0"]:L["m0"] + 4]).view(L["mtype"]).reshape(-1)
    assert np.array_equal(gm, om), (fam, where, gm, om)
    used = np.zeros(L["stride"], bool)
    used[L["b0"]:L["b0"] + L["nb"]] = True
    used[L["m0"]:L["m0"] + 4] = True
    assert not got[:, ~used].any(), (fam, where)
    if L["zero_tail"]:
        assert not cand_i[no:].any(), (fam, where)
    else:
        assert untouched(cand_i[no:]), (fam, where)


def check_list(fam, n, w, cand, cnt, exps, where=None):
    """a whole sparse launch: cand [n + 1][K][stride], cnt [n + 1] (int32, pre-filled with -1), exps[i] = oracle_list of item i (needed
    where decoded_mask says so); item n is the guard"""
    dm = decoded_mask(fam, w)
    for i in range(n):
        check_list_item(fam, cand[i], cnt[i], exps[i] if dm[i] else None, bool(dm[i]), (where, i))
    assert cnt[n] == -1 and untouched(cand[n]), (fam, where, "guard")


def check_rows(n, rows_wanted, G, out, nby, exp_out, unwanted, where=None, extra=None):
    """row decoders (k5_nxdn, k5_m17, greedy): out [n + 1][stride] u8, the first nby bytes of a row are the decoder's.  A wanted row is the
    oracle's; an unwanted row beside a wanted one (same group of G; G = 1: never) is decoded as well; an unwanted row in an empty group
    reads `unwanted` ('zero' or 'kept').  Bytes beyond nby are left alone unless the kernel zero-fills the stride (extra = 'zero').
    -> which rows were decoded"""
    rows_wanted = np.asarray(rows_wanted, bool)
    dec = group_has_wanted(rows_wanted, G) if G > 1 else rows_wanted
    for i in range(n):
        if dec[i]:
            assert np.array_equal(out[i, :nby], exp_out[i, :nby]), (where, i)
            assert (not out[i, nby:].any()) if extra == "zero" else untouched(out[i, nby:]), (where, i)
        else:
            assert (not out[i, :nby].any()) if unwanted == "zero" else untouched(out[i, :nby]), (where, i)
            assert untouched(out[i, nby:]), (where, i)
    assert untouched(out[n]), (where, "guard")
    return dec


def expected_pick(td, rel, hard, soft, cands, n_list):
    """one burst of k_dmr_r34_pick from the product's own decodes (hard18, soft18, the list's candidates [32][24], the count the kernel is
    given) -> (pool24 [pool_n][24] as the kernel lays it out, unconf18, conf18, conf_crc)"""
    nl = min(int(n_list), 32)
    pool, n_hs = dmr_data.pool_of(td, rel, [hard, soft] + [cands[j, 4:22] for j in range(nl)])
    p24 = np.zeros((len(pool), 24), np.uint8)
    for k, (b, metric, crc, dbsn) in enumerate(pool):
        p24[k, 0:4] = np.array([metric], np.int32).view(np.uint8)
        p24[k, 4:22] = b
        p24[k, 22] = crc
        p24[k, 23] = dbsn
    u = dmr_data.pick_unconfirmed(pool, n_hs)
    c, crc = dmr_data.pick_confirmed(pool)
    return p24, pool[u][0], pool[c][0], crc


# ---- the device entries (extern "C", not hidden): prototypes on a handle of this module's own ---------------------------------------
_dev = None


def dev():
    """libdsdneo_hip.so with argtypes for the internal entries the sparse tests call (device pointers as integers, hipStream_t as a
    pointer); a handle of its own, so the public prototypes of bindings/ddn.py stay as they are"""
    global _dev
    if _dev is None:
        import ddn
        ddn.lib()                            # (loads torch's HIP runtime first)
        l = C.CDLL(ddn.LIB_PATH)
        I, Z = C.c_int, C.c_size_t
        protos = {
            "ddn_dev_p25_half_rate_list_wanted": (I, [VP, I, I, VP, VP, VP, VP]),
            "ddn_dev_p25_half_rate_list_wanted_wide": (I, [VP, I, I, VP, VP, VP, VP]),
            "ddn_dev_r34_list_wanted": (I, [VP, VP, I, I, VP, VP, VP, VP, VP]),
            "ddn_dev_k5_nxdn_wanted": (I, [VP, VP, I, I, I, VP, VP, I, VP, I, VP]),
            "ddn_dev_trellis_greedy_wanted": (I, [VP, I, Z, I, VP, I, VP, VP]),
            "ddn_dev_dmr_r34_pick": (I, [VP, VP, VP, VP, VP, VP, VP, I, VP, VP, VP, VP, VP, VP]),
            "ddn_fec_viterbi_k5_batch_wanted": (I, [VP, Z, I, VP, I, VP, I, VP, VP, VP]),
            "ddn_fec_p25_mbf34_list_batch": (I, [VP, Z, I, VP, VP, VP, VP]),
            "ddn_fec_r34_batch": (I, [VP, VP, Z, VP, VP]),
            "ddn_fec_r34_list_batch": (I, [VP, VP, Z, I, VP, VP, VP]),
            "ddn_fec_nxdn_conv_batch": (I, [VP, VP, Z, I, I, VP, VP, I, VP]),
            "ddn_last_error": (C.c_char_p, []),
        }
        for name, (res, args) in protos.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _dev = l
    return _dev


def nxdn_lds_bytes(n_steps, soft):
    """the dynamic LDS k_k5_nxdn asks for: 16 code words of symbols (and reliabilities), 16 decision words per step, 16 spare"""
    return 16 * (2 * n_steps + 2) * (2 if soft else 1) + 32 * n_steps + 16
