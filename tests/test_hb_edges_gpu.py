"""GPU: the half-band decimators at their edges.  The drop-ins simd_hb_decim2_real / simd_hb_decim2_complex against the oracle at
the block lengths of tests/test_oracle_hb_real.py (where the oracle itself is held to the compiled reference), and the batched
cascade of ddn_batch_set_decimation with last blocks of a few samples: the non-fused branch of k_hb_decim2, odd stage lengths,
output counts off the reference's vector width, an LPF block shorter than its taps.  Bit for bit: outputs, return values, carried
history; the words behind the last output stay untouched."""
import ctypes as C

import numpy as np
import pytest

import cs16
import ddn
import hb_edge
import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fns(built):
    o, l = orc.oracle(), ddn.lib()
    o.orc_hb_decim2_real.restype = C.c_int
    o.orc_hb_decim2_real.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return o, l


@pytest.mark.parametrize("kind", ["noise", "zeros"])
@pytest.mark.parametrize("nt", [15, 31, 23])
def test_real_dropin_at_every_edge_length(fns, nt, kind):
    o, l = fns
    taps = hb_edge.tap_sets()[nt]
    for n in hb_edge.REAL_LENS:
        xs = hb_edge.calls(kind, 1000 * nt + n, n, 1)
        h0 = hb_edge.history(kind, n, nt - 1)
        want = hb_edge.run_real(o.orc_hb_decim2_real, xs, taps, h0, 1)
        got = hb_edge.run_real(l.simd_hb_decim2_real, xs, taps, h0)
        assert all(w[0] == n // 2 for w in want)
        assert hb_edge.same(got, want), (n, hb_edge.first_difference(got, want))


@pytest.mark.parametrize("kind", ["noise", "zeros"])
@pytest.mark.parametrize("nt", [15, 31, 23])
def test_complex_dropin_at_every_edge_length(fns, nt, kind):
    o, l = fns
    taps = hb_edge.tap_sets()[nt]
    for n in hb_edge.COMPLEX_LENS:
        xs = hb_edge.calls(kind, 2000 * nt + n, n, 2)
        hi, hq = hb_edge.history(kind, n, nt - 1), hb_edge.history(kind, n + 1, nt - 1)
        want = hb_edge.run_complex(o.orc_hb_decim2_complex, xs, taps, hi, hq, 1)
        got = hb_edge.run_complex(l.simd_hb_decim2_complex, xs, taps, hi, hq)
        assert all(w[0] == 2 * (n // 2) for w in want)
        assert hb_edge.same(got, want), (n, hb_edge.first_difference(got, want))


@pytest.mark.parametrize("form", ["real", "complex"])
@pytest.mark.parametrize("nt", [15, 31, 23])
def test_dropins_on_the_built_windows(fns, nt, form):
    """the windows of hb_edge.edge_window (every product a negative zero), aimed at both ends of the prefix, of the vector span and
    of the scalar tail - tests/test_oracle_hb_real.py holds on the reference's own output that these give +0.0 at a vector output
    and -0.0 at a scalar-helper one: the drop-in gives that sign there and equals the oracle over the whole call"""
    o, l = fns
    taps = hb_edge.tap_sets()[nt]
    cx = form == "complex"
    n = hb_edge.EDGE_COMPLEX_LEN if cx else hb_edge.EDGE_REAL_LEN
    targets = hb_edge.edge_outputs(nt, n, cx)
    assert {v for _, v in targets} == {True, False} and len(targets) >= 4
    for m, vector in targets:
        x, hist = hb_edge.edge_window(taps, n, m, 100 * nt + m, cx)
        if cx:
            want = hb_edge.run_complex(o.orc_hb_decim2_complex, [x], taps, *hist, 1)
            got = hb_edge.run_complex(l.simd_hb_decim2_complex, [x], taps, *hist)
            at = got[0][1][2 * m:2 * m + 2]
        else:
            want = hb_edge.run_real(o.orc_hb_decim2_real, [x], taps, *hist, 1)
            got = hb_edge.run_real(l.simd_hb_decim2_real, [x], taps, *hist)
            at = got[0][1][m:m + 1]
        assert hb_edge.is_zero_of_sign(at, negative=not vector), (m, vector, at)
        assert hb_edge.same(got, want), (m, hb_edge.first_difference(got, want))


def test_channel_filter_dropin_at_the_scalar_tail(fns):
    """simd_fir_complex_apply against the oracle (held to the compiled reference in tests/test_oracle_hb_real.py) at lengths of every
    n % 4, three calls with one carried history, and on the built windows: -0.0 at the last n % 4 outputs, +0.0 before them"""
    o, l = fns
    for taps in hb_edge.channel_taps():
        nt = len(taps)
        for n in (1, 5, nt - 1, nt, nt + 2, 1200, 1201, 1202, 1203):
            xs = hb_edge.calls("zeros", 7 * nt + n, n, 2)
            hi, hq = hb_edge.history("noise", n, nt - 1), hb_edge.history("zeros", n + 1, nt - 1)
            want = hb_edge.run_fir(o.orc_fir_complex_apply, xs, taps, hi, hq, 1)
            got = hb_edge.run_fir(l.simd_fir_complex_apply, xs, taps, hi, hq)
            assert hb_edge.same(got, want), (nt, n, hb_edge.first_difference(got, want))
        n = hb_edge.EDGE_FIR_LEN
        for m, vector in hb_edge.fir_edge_outputs(n):
            x, hist = hb_edge.edge_window(taps, n, m, nt + m, True, stride=1)
            want = hb_edge.run_fir(o.orc_fir_complex_apply, [x], taps, *hist, 1)
            got = hb_edge.run_fir(l.simd_fir_complex_apply, [x], taps, *hist)
            assert hb_edge.is_zero_of_sign(got[0][1][2 * m:2 * m + 2], negative=not vector), (nt, m, vector)
            assert hb_edge.same(got, want), (nt, m, hb_edge.first_difference(got, want))


def test_real_dropin_refuses_what_the_reference_refuses(fns):
    o, l = fns
    x, out, h, taps = np.ones(8, np.float32), np.full(8, 7.0, np.float32), np.ones(14, np.float32), hb_edge.tap_sets()[15]
    for in_len, nt in ((0, 15), (-2, 15), (8, 14), (8, 1)):
        assert l.simd_hb_decim2_real(x.ctypes.data, in_len, out.ctypes.data, h.ctypes.data, taps.ctypes.data, nt) == 0
    assert (out == 7.0).all() and (h == 1.0).all()


B, BLK = 6, 1200
TAILS = (1, 3, 7, 11, 17)


def _input(fmt, passes, n):
    """-> (the array the batch takes, the per-channel arrays its oracle takes, the oracle's run method)"""
    u8 = orc.synth_c4fm_cu8(40, B, n, sps=10 << passes)
    if fmt == "cu8":
        return u8, u8, "run_cu8"
    if fmt == "cs16":
        x = cs16.cu8_to_cs16(u8)
        return x, cs16.widen(x), "run_f32"
    f = ((u8.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 127.5)).astype(np.float32)
    # cf32 alone can carry signed zeros: runs of them, so that whole windows of the first stages are zeros
    rng = np.random.default_rng(passes)
    for c in range(B):
        for p in range(100 + 37 * c, n - 200, 900):
            f[c, p:p + 150] = np.where(rng.random((150, 2)) < 0.75, np.float32(-0.0), np.float32(0.0))
    f[:, -40:] = np.float32(-0.0)
    return f, f, "run_f32"


@pytest.mark.parametrize("fmt", ["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("passes", [1, 2, 3])
def test_cascade_with_last_blocks_of_a_few_samples(built, passes, fmt):
    fmt_id = {"cu8": ddn.IN_CU8, "cs16": ddn.IN_CS16, "cf32": ddn.IN_CF32}[fmt]
    for t in TAILS:
        tail = t << passes
        calls = [BLK + tail, 2 * BLK + tail, tail]      # the last call is nothing but the short block
        n = sum(calls)
        x, w, run = _input(fmt, passes, n)
        b = ddn.Batch(B, block_len=BLK, input_format=fmt_id)
        b.set_decimation(passes)
        got, pos = [], 0
        for ln in calls:
            got.append(b.run_host(np.ascontiguousarray(x[:, pos:pos + ln]), ln))
            pos += ln
        for c in range(B):
            fe = orc.OracleFrontEnd(downsample_passes=passes)
            pos = 0
            for k, ln in enumerate(calls):
                want = getattr(fe, run)(np.ascontiguousarray(w[c, pos:pos + ln]), BLK)
                assert len(want) == ln >> passes == got[k].shape[1], (t, k, len(want))
                assert np.array_equal(got[k][c].view(np.uint32), want.view(np.uint32)), (t, c, k)
                pos += ln
            assert cs16.same_bits(b.fsk_state(c), cs16.oracle_fsk_state(fe)), (t, c)
        b.close()
