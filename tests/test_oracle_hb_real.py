"""CPU: the oracle's half-band decimators (oracle/ddn_oracle_dsp.c: orc_hb_decim2_real, orc_hb_decim2_complex) against the compiled
reference's simd_hb_decim2_real / simd_hb_decim2_complex, bit for bit, at the block lengths where the reference changes unit or
order: both sides of 2 * taps_len (the dispatcher's scalar rule), blocks shorter than the history, odd lengths, and every count
of outputs the AVX2 unit leaves to its scalar helpers.  Three calls with one carried history.  Skipped where oracle/_ref was not
built."""
import ctypes as C

import numpy as np
import pytest

import hb_edge
import orc


@pytest.fixture(scope="module")
def libs(built):
    r = orc.ref()
    if r is None:
        pytest.skip("oracle/_ref not built")
    assert r.simd_fir_get_impl_name() == b"avx2"        # the unit the oracle's fma_order = 1 restates
    o = orc.oracle()
    o.orc_hb_decim2_real.restype = C.c_int
    o.orc_hb_decim2_real.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    r.simd_hb_decim2_real.restype = C.c_int
    r.simd_hb_decim2_real.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    r.simd_hb_decim2_complex.restype = C.c_int
    r.simd_hb_decim2_complex.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return o, r


@pytest.mark.parametrize("kind", ["noise", "zeros"])
@pytest.mark.parametrize("nt", [15, 31, 23])
def test_real_halfband_oracle_equals_the_reference(libs, nt, kind):
    o, r = libs
    taps = hb_edge.tap_sets()[nt]
    for n in hb_edge.REAL_LENS:
        xs = hb_edge.calls(kind, 1000 * nt + n, n, 1)
        h0 = hb_edge.history(kind, n, nt - 1)
        want = hb_edge.run_real(r.simd_hb_decim2_real, xs, taps, h0)
        got = hb_edge.run_real(o.orc_hb_decim2_real, xs, taps, h0, 1)
        assert all(w[0] == n // 2 for w in want)
        assert hb_edge.same(got, want), (n, hb_edge.first_difference(got, want))


@pytest.mark.parametrize("kind", ["noise", "zeros"])
@pytest.mark.parametrize("nt", [15, 31, 23])
def test_complex_halfband_oracle_equals_the_reference(libs, nt, kind):
    o, r = libs
    taps = hb_edge.tap_sets()[nt]
    for n in hb_edge.COMPLEX_LENS:
        xs = hb_edge.calls(kind, 2000 * nt + n, n, 2)
        hi, hq = hb_edge.history(kind, n, nt - 1), hb_edge.history(kind, n + 1, nt - 1)
        want = hb_edge.run_complex(r.simd_hb_decim2_complex, xs, taps, hi, hq)
        got = hb_edge.run_complex(o.orc_hb_decim2_complex, xs, taps, hi, hq, 1)
        assert all(w[0] == 2 * (n // 2) for w in want)
        assert hb_edge.same(got, want), (n, hb_edge.first_difference(got, want))


@pytest.mark.parametrize("form", ["real", "complex"])
@pytest.mark.parametrize("nt", [15, 31, 23])
def test_built_windows_tell_the_two_orders_apart(libs, nt, form):
    """one window built so that every product is a negative zero (hb_edge.edge_window), aimed in turn at both ends of the prefix, of
    the vector span and of the scalar tail: the reference returns +0.0 where its vector loop computes the output and -0.0 where a
    scalar helper does - asserted on the reference's own output - and the oracle equals it bit for bit, so which outputs start
    from the plain centre product is pinned for every tap set and both forms, not left to what random zero runs happen to hit"""
    o, r = libs
    taps = hb_edge.tap_sets()[nt]
    cx = form == "complex"
    n = hb_edge.EDGE_COMPLEX_LEN if cx else hb_edge.EDGE_REAL_LEN
    targets = hb_edge.edge_outputs(nt, n, cx)
    assert {v for _, v in targets} == {True, False} and len(targets) >= 4
    for m, vector in targets:
        x, hist = hb_edge.edge_window(taps, n, m, 100 * nt + m, cx)
        if cx:
            want = hb_edge.run_complex(r.simd_hb_decim2_complex, [x], taps, *hist)
            got = hb_edge.run_complex(o.orc_hb_decim2_complex, [x], taps, *hist, 1)
            at = want[0][1][2 * m:2 * m + 2]
        else:
            want = hb_edge.run_real(r.simd_hb_decim2_real, [x], taps, *hist)
            got = hb_edge.run_real(o.orc_hb_decim2_real, [x], taps, *hist, 1)
            at = want[0][1][m:m + 1]
        assert hb_edge.is_zero_of_sign(at, negative=not vector), (m, vector, at)
        assert hb_edge.same(got, want), (m, hb_edge.first_difference(got, want))


def test_channel_filter_oracle_equals_the_reference_at_the_scalar_tail(libs):
    """orc_fir_complex_apply (the channel low-pass of every front-end oracle) against the compiled simd_fir_complex_apply: three
    calls of noise at lengths of every n % 4 with one carried history, and the built windows - +0.0 from the reference where its
    vector loops compute the output, -0.0 from the helper that takes the last n % 4 outputs - asserted on the reference's output"""
    o, r = libs
    r.simd_fir_complex_apply.restype = None
    r.simd_fir_complex_apply.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    for taps in hb_edge.channel_taps():
        nt = len(taps)
        for n in (1, 5, nt - 1, nt, nt + 2, 1200, 1201, 1202, 1203):
            xs = hb_edge.calls("zeros", 7 * nt + n, n, 2)
            hi, hq = hb_edge.history("noise", n, nt - 1), hb_edge.history("zeros", n + 1, nt - 1)
            want = hb_edge.run_fir(r.simd_fir_complex_apply, xs, taps, hi, hq)
            got = hb_edge.run_fir(o.orc_fir_complex_apply, xs, taps, hi, hq, 1)
            assert hb_edge.same(got, want), (nt, n, hb_edge.first_difference(got, want))
        n = hb_edge.EDGE_FIR_LEN
        for m, vector in hb_edge.fir_edge_outputs(n):
            x, hist = hb_edge.edge_window(taps, n, m, nt + m, True, stride=1)
            want = hb_edge.run_fir(r.simd_fir_complex_apply, [x], taps, *hist)
            got = hb_edge.run_fir(o.orc_fir_complex_apply, [x], taps, *hist, 1)
            assert hb_edge.is_zero_of_sign(want[0][1][2 * m:2 * m + 2], negative=not vector), (nt, m, vector)
            assert hb_edge.same(got, want), (nt, m, hb_edge.first_difference(got, want))
