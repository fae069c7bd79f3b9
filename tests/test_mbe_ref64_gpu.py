"""GPU: k_mbe_params / k_mbe_synth (dsd-neo_amd/csrc/ddn_mbe.hip) held to the float64 model of tests/mbe_ref64.py - the cases,
bounds and checks of tests/test_mbe_ref64.py, driven through ddn_mbe_batch_set_state / _get_state and repeat frames, so the
device's synthesis, enhancement and phase track are compared with something that is not a copy of themselves.  The
derivation of the bounds is in tests/mbe_ref64.py and in the docstrings of tests/test_mbe_ref64.py."""
import ctypes as C

import numpy as np
import pytest

import ddn
import test_mbe_ref64 as T
from test_mbe_gpu import GpuVocoder

pytestmark = pytest.mark.gpu


class GpuDriver:
    def __init__(self, codec, S, first_stream=0):
        self.g = GpuVocoder(codec, S)
        if first_stream:
            assert ddn.lib().ddn_mbe_batch_set_first_stream(self.g.h, first_stream, None) == 0

    def set_state(self, s, cur, prev, enh):
        assert ddn.lib().ddn_mbe_batch_set_state(self.g.h, s, C.byref(cur), C.byref(prev), C.byref(enh)) == 0

    def state(self, s):
        return self.g.state(s)

    def run(self, bits, res_in=None):
        return self.g.run(np.ascontiguousarray(bits), res_in)


@pytest.fixture(scope="module")
def cases():
    return T.build_cases()


@pytest.fixture(scope="module")
def gpu_runs(built, cases):
    return {codec: T.run_repeat_batch(GpuDriver, codec, cases) for codec in T.CODECS}


@pytest.mark.parametrize("codec", T.CODECS)
def test_synth_against_float64(gpu_runs, cases, codec):
    """|pcm[n] - ref[n]| <= 2^-14 A[n] + 2^-20 on all 160 samples (55/56 and 104/105, where a lane's three stretches meet, included)
    of the 96 chosen states, talk paths 0..95, and of eight of them behind a non-zero ddn_mbe_batch_set_first_stream.
    Measured on an MI355X: worst |d| / A = 1.29e-5, 0.21 of the bound (the restatement's figure: the device equals it bit for bit)."""
    fig = T.check_repeat_synth(codec, cases, *gpu_runs[codec])
    few = cases[:8]
    T.check_repeat_synth(codec, few, *T.run_repeat_batch(GpuDriver, codec, few, T.FIRST_STREAM))
    assert fig["synth |d|/A (absolute figure)"] > 2.0 ** -26


@pytest.mark.parametrize("codec", T.CODECS)
def test_enhancement_and_phase_against_float64(gpu_runs, cases, codec):
    """prev_enhanced.Ml within 2^-18 relative of enhance() of the amplitudes that were set, the energy kept within 2^-18, PSIl and
    PHIl within 2^-11 rad of phases() circularly (the sum is spelled out in tests/test_mbe_ref64.py), PSIl in [-pi, pi].
    Measured on an MI355X: enhancement 0.08 of its bound, energy 0.11, PSIl and PHIl 0.73; no harmonic skipped."""
    pcm, before, after, seeds = gpu_runs[codec]
    T.check_repeat_enhance_phase(codec, cases, before, after, seeds)


def test_three_repeats_keep_phase_and_counter(built):
    """three repeat frames as one call of three and as three calls of one: the same PCM bit for bit; the frame counter, the repeat
    count, the phase track and the hash's frame number (f, f + 1, f + 2) continue; PCM of frames 2 and 3 within the bound with the
    previous side taken from the state read back"""
    T.run_three_repeats(GpuDriver)


@pytest.mark.parametrize("codec", T.CODECS)
def test_decoded_frames_against_float64(built, codec):
    """8 paths x 6 ordinary random frames, one frame per call, the states read around each call: synthesis, enhancement and phases as
    above, and prev.Ml within 2^-20 relative of ml_from_log2(prev.log2Ml).
    Measured on an MI355X (IMBE / AMBE): synthesis 0.26 / 0.10 of the bound (|d| / A = 1.56e-5 / 6.2e-6), Ml 0.49 / 0.34,
    enhancement 0.98 / 0.08 (the 0.98 is one ill-conditioned harmonic, see tests/test_mbe_ref64.py; the next is at 0.35)"""
    T.run_decoded_frames(GpuDriver, codec)
