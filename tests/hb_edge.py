"""Shared cases of the half-band edge tests (tests/test_oracle_hb_real.py on the CPU, tests/test_hb_edges_gpu.py on the device):
tap sets, block lengths, the two input kinds and the windows built to tell the reference's two accumulation orders apart.  TEST INFRASTRUCTURE - never imported by the product."""
import ctypes as C

import numpy as np

import orc

# real in_len: both sides of 2 * taps_len for 15 and 31 taps, shorter than the history, odd lengths, every out_len % 8
REAL_LENS = (1, 2, 3, 13, 29, 30, 61, 62, 63, 77, 6001, 6002, 6007, 6015)
# complex samples per call (in_len = 2 * ch_len)
COMPLEX_LENS = (1, 2, 3, 15, 30, 31, 33, 3001, 3002, 3003, 3005, 3007)


def tap_sets():
    o = orc.oracle()
    hb31 = np.ctypeslib.as_array((C.c_float * 31).in_dll(o, "orc_hb31_taps")).copy()
    hb15 = np.ctypeslib.as_array((C.c_float * 15).in_dll(o, "orc_hb15_taps")).copy()
    # 23 taps: the Hamming-windowed set of test_front_end_gpu.py::test_dropin_symbols_match_oracle
    k = np.arange(23) - 11
    hb23 = np.where(k == 0, 0.5, np.where(k % 2 != 0, np.sin(np.pi * k / 2) / (np.pi * np.where(k == 0, 1, k)), 0.0))
    hb23 = (hb23 * np.hamming(23)).astype(np.float32)
    return {15: hb15, 31: hb31, 23: hb23}


def stream(kind, rng, n):
    """n float32 samples.  "noise": Gaussian.  "zeros": Gaussian with runs of signed zeros, three in four of them negative, each
    run longer than the longest tap set - inside a run every product of a window is a zero, and its sign depends on the signs of
    the tap and of the two partners, so an output of -0.0 (centre product first) or +0.0 (FMA onto +0.0) tells the orders apart"""
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "zeros":
        z = np.where(rng.random(n) < 0.75, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        pos = 0
        while pos < n:
            run = int(rng.integers(40, 160))
            if rng.random() < 0.7:
                x[pos:pos + run] = z[pos:pos + run]
            pos += run
        x[-3:] = np.float32(-0.0)                       # the replicated last sample is a negative zero too
    return x


def calls(kind, seed, n, width):
    """three calls of n * width floats each (width 1: real, 2: interleaved complex)"""
    rng = np.random.default_rng(seed)
    return [stream(kind, rng, n * width) for _ in range(3)]


def run_real(fn, xs, taps, hist0, *extra):
    """fn(in, in_len, out, hist, taps, taps_len, *extra) over the calls xs with one carried history -> [(ret, out, hist)]"""
    hist = hist0.copy()
    res = []
    for x in xs:
        out = np.full(len(x) // 2 + 8, 7.0, np.float32)
        r = fn(x.ctypes.data, len(x), out.ctypes.data, hist.ctypes.data, taps.ctypes.data, len(taps), *extra)
        res.append((r, out.copy(), hist.copy()))
    return res


def run_complex(fn, xs, taps, hist0_i, hist0_q, *extra):
    hi, hq = hist0_i.copy(), hist0_q.copy()
    res = []
    for x in xs:
        out = np.full(len(x) // 2 + 8, 7.0, np.float32)
        r = fn(x.ctypes.data, len(x), out.ctypes.data, hi.ctypes.data, hq.ctypes.data, taps.ctypes.data, len(taps), *extra)
        res.append((r, out.copy(), hi.copy(), hq.copy()))
    return res


def same(a, b):
    """bit for bit: return code, every output word (the untouched guard words behind it too) and the carried history"""
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        if ra[0] != rb[0]:
            return False
        for u, v in zip(ra[1:], rb[1:]):
            if not np.array_equal(u.view(np.uint32), v.view(np.uint32)):
                return False
    return True


def first_difference(a, b):
    for k, (ra, rb) in enumerate(zip(a, b)):
        if ra[0] != rb[0]:
            return "call %d: returned %d, want %d" % (k, ra[0], rb[0])
        for j, (u, v) in enumerate(zip(ra[1:], rb[1:])):
            bad = np.flatnonzero(u.view(np.uint32) != v.view(np.uint32))
            if bad.size:
                return "call %d, array %d, index %d of %d: %r != %r" % (k, j, bad[0], ra[0], u[bad[0]], v[bad[0]])
    return None


def history(kind, seed, n):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n).astype(np.float32)
    if kind == "zeros":
        h[n // 2:] = np.float32(-0.0)
    return h


# ---- one window built on purpose -------------------------------------------------------------------------------------------------------
# The reference's AVX2 units start an output of their vector loops with an FMA onto +0.0 and an output of their scalar helpers with
# the plain centre product.  The two agree unless every product of the window is a zero: negative zeros under the centre and the
# positive taps, and one +0.0 partner under each negative tap, make every product -0.0 - the helper then returns -0.0, the vector
# loop +0.0.  One window per call, so that neighbouring windows do not ask for contradicting signs.
EDGE_REAL_LEN = 6015         # 3007 outputs: 3000 in the eight-wide loop, seven behind it (four of them inside a four-wide loop's reach)
EDGE_COMPLEX_LEN = 3005      # 1502 outputs: not a multiple of four, and six past a multiple of eight


def vector_span(nt, n, is_complex):
    """[begin, end): the outputs of a block of n samples (per channel) that the AVX2 unit computes in its vector loop - real: eight
    per step from output 0; complex with 15 / 31 taps: after the outputs whose window reaches the history, eight per step while
    the step's loads stay inside the block; complex with other lengths: four per step from output 0"""
    n_out, cen = n // 2, (nt - 1) // 2
    if not is_complex:
        return 0, n_out & ~7
    if nt not in (15, 31):
        return 0, n_out & ~3
    i = begin = min((cen + 1) // 2, n_out)
    while i + 7 < n_out and 2 * i + cen + 15 < n:
        i += 8
    return begin, i


def edge_outputs(nt, n, is_complex):
    """the outputs to aim a window at -> [(output index, True if the vector loop computes it)]: both ends of the prefix, of the
    vector span and of the scalar tail"""
    begin, end = vector_span(nt, n, is_complex)
    n_out = n // 2
    picks = {0, begin - 1, begin, (begin + end) // 2, end - 1, end, n_out - 1}
    return [(m, begin <= m < end) for m in sorted(picks) if 0 <= m < n_out]


def edge_window(taps, n, m, seed, is_complex, stride=2):
    """-> (x, [history per channel]): Gaussian noise with the window of output m set as described above (I and Q alike).  stride 2:
    a half-band decimator (centre on sample 2 m, every other tap); stride 1: the plain symmetric filter (centre on sample m)"""
    nt = len(taps)
    cen, hist_len = (nt - 1) // 2, nt - 1
    rng = np.random.default_rng(seed)
    line = rng.standard_normal(hist_len + n).astype(np.float32)     # history, then the block: sample j of the block at hist_len + j
    c = hist_len + stride * m
    line[c] = np.float32(-0.0)
    for k in range(0, cen, stride):
        d = cen - k
        if taps[k] == 0.0:
            continue
        line[c - d] = np.float32(0.0) if taps[k] < 0.0 else np.float32(-0.0)
        if c + d < hist_len + n:
            line[c + d] = np.float32(-0.0)
        else:
            line[hist_len + n - 1] = np.float32(-0.0)               # (the block's last sample stands in for what lies behind it)
    assert taps[cen] > 0.0
    hist, x = line[:hist_len].copy(), line[hist_len:].copy()
    if is_complex:
        return np.ascontiguousarray(np.repeat(x, 2)), [hist, hist.copy()]
    return x, [hist]


def is_zero_of_sign(v, negative):
    v = np.asarray(v, np.float32)
    return bool((v == 0.0).all() and (np.signbit(v) == negative).all())


# ---- the plain symmetric complex filter (simd_fir_complex_apply: the channel low-pass) ---------------------------------------------------
EDGE_FIR_LEN = 3007          # complex samples: the AVX2 unit takes eight, then four per step - 3004 in all - and leaves three to its helper


def fir_edge_outputs(n):
    end = n & ~3
    return [(m, m < end) for m in sorted({0, end // 2, end - 1, end, n - 1})]


def run_fir(fn, xs, taps, hist0_i, hist0_q, *extra):
    """fn(in, in_len, out, hist_i, hist_q, taps, taps_len, *extra) over the calls xs -> [(0, out, hist_i, hist_q)]"""
    hi, hq = hist0_i.copy(), hist0_q.copy()
    res = []
    for x in xs:
        out = np.full(len(x) + 8, 7.0, np.float32)
        fn(x.ctypes.data, len(x), out.ctypes.data, hi.ctypes.data, hq.ctypes.data, taps.ctypes.data, len(taps), *extra)
        res.append((0, out.copy(), hi.copy(), hq.copy()))
    return res


def channel_taps():
    """the 135-tap P25 C4FM channel filter at 48 kHz and the 67-tap 6.25 kHz one at 24 kHz"""
    out = []
    for rate, profile in ((48000, 4), (24000, 1)):
        t = np.zeros(144, np.float32)
        nt = orc.oracle().orc_channel_lpf_design(rate, profile, t.ctypes.data, 144)
        out.append(t[:nt].copy())
    return out
