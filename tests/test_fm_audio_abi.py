"""The analog FM monitor's C ABI where no device is needed: argument checks, and the count rule (ddn_fm_audio_plan, the rule
ddn_fm_audio_run returns its count by) against the restatement's counts.  The checks that need a batch are in test_fm_audio_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import ddn
import fm_audio


def plan(ac, passes, block_len, n, phase, idx):
    ph, ix, cnt = C.c_int(phase), C.c_int(idx), C.c_size_t(0)
    rc = ddn.lib().ddn_fm_audio_plan(C.byref(ac), passes, block_len, n, C.byref(ph), C.byref(ix), C.byref(cnt))
    return rc, cnt.value, ph.value, ix.value


def test_null_arguments_and_bad_configurations(built):
    l = ddn.lib()
    ac = ddn.FmAudioConfig()
    cnt = C.c_size_t(0)
    buf = np.zeros(64, np.float32)
    assert l.ddn_batch_set_audio_monitor(None, C.byref(ac)) == ddn.DDN_EINVAL
    assert l.ddn_fm_audio_max_samples(None, 100) == 0
    assert l.ddn_fm_audio_run(None, buf.ctypes.data, 8, buf.ctypes.data, 8, C.byref(cnt), None) == ddn.DDN_EINVAL
    assert l.ddn_fm_audio_host_run(None, buf.ctypes.data, 8, buf.ctypes.data, 8, C.byref(cnt)) == ddn.DDN_EINVAL
    assert b"ddn_fm_audio_host_run" in l.ddn_last_error()
    assert l.ddn_batch_get_audio_coefficients(None, buf.ctypes.data, buf.ctypes.data) == ddn.DDN_EINVAL
    assert l.ddn_batch_get_audio_state(None, 0, buf.ctypes.data) == ddn.DDN_EINVAL
    assert l.ddn_fm_audio_design(48000, None, buf.ctypes.data, buf.ctypes.data) == ddn.DDN_EINVAL
    assert l.ddn_fm_audio_design(48000, C.byref(ac), None, buf.ctypes.data) == ddn.DDN_EINVAL
    for bad in (dict(deemph_tau_us=60), dict(audio_lpf_cutoff_hz=-1), dict(squelch_env_attack=-0.5), dict(squelch_env_release=float("nan"))):
        assert l.ddn_fm_audio_design(48000, C.byref(ddn.FmAudioConfig(**bad)), buf.ctypes.data, buf[16:].ctypes.data) == ddn.DDN_EINVAL, bad
    # low_pass_real above its input rate: the reference's index grows without bound
    assert l.ddn_fm_audio_design(48000, C.byref(ddn.FmAudioConfig(lpr_fast_hz=8000, lpr_slow_hz=48000)), buf.ctypes.data,
                                 buf[16:].ctypes.data) == ddn.DDN_ERANGE
    assert b"lpr_slow_hz" in l.ddn_last_error()


def test_design_defaults(built):
    """all zero = the reference's analog defaults: no decimator, DC block on, 2^-11; deemph on -> tau 75 us, the Q15-rounded coefficient"""
    c3, t16 = np.ones(3, np.float32), np.ones(16, np.float32)
    assert ddn.lib().ddn_fm_audio_design(48000, C.byref(ddn.FmAudioConfig()), c3.ctypes.data, t16.ctypes.data) == 0
    assert c3.tolist() == [0.0, 0.0, 2.0 ** -11] and not t16.any()
    assert ddn.lib().ddn_fm_audio_design(48000, C.byref(ddn.FmAudioConfig(deemph=1, audio_lpf_cutoff_hz=5, post_downsample=3)), c3.ctypes.data,
                                         t16.ctypes.data) == 0
    assert c3[1] == np.float32(1 - np.exp(-2 * np.pi * 100 / 48000))           # a cutoff below 100 Hz is 100 Hz
    assert abs(float(t16.astype(np.float64).sum()) - 1.0) < 1e-6 and int(np.argmax(t16)) == 7   # unit gain, centred on (K - 1) / 2


@pytest.mark.parametrize("rate", [8000, 12000, 24000, 48000, 96000])
def test_design_coefficients_exactly(built, rate):
    """deemph_a is round-to-nearest(alpha 2^15) / 2^15 exactly, alpha = 1 - e^(-1 / (rate tau)) in binary64, for the three time constants
    (0 = 75 us); the audio LPF's alpha is the binary32 rounding of 1 - e^(-2 pi fc / rate), fc below 100 Hz taken as 100.  (The compiled
    reference does not hold the unit these come from; this is the arithmetic of its source restated with numpy's binary64.)"""
    c3, t16 = np.zeros(3, np.float32), np.zeros(16, np.float32)
    for tau_us, tau in ((0, 75e-6), (50, 50e-6), (75, 75e-6), (750, 750e-6)):
        for cutoff in (1, 100, 300, 3000, 5000):
            ac = ddn.FmAudioConfig(deemph=1, deemph_tau_us=tau_us, audio_lpf_cutoff_hz=cutoff)
            assert ddn.lib().ddn_fm_audio_design(rate, C.byref(ac), c3.ctypes.data, t16.ctypes.data) == 0
            alpha = np.float64(1.0) - np.exp(np.float64(-1.0) / (np.float64(rate) * np.float64(tau)))
            q15 = min(max(int(np.rint(alpha * 32768.0)), 1), 32767)                # rint: to nearest, ties to even, like lrint
            assert abs(alpha * 32768.0 - np.rint(alpha * 32768.0)) < 0.49          # (no tie in these cases: the direction is decided)
            assert float(c3[0]) == q15 / 32768.0, (rate, tau_us, float(c3[0]) * 32768, q15)
            g = np.float64(1.0) - np.exp(np.float64(-2.0) * np.float64(np.pi) * np.float64(max(cutoff, 100)) / np.float64(rate))
            assert c3[1] == np.float32(min(max(g, 0.0), 1.0)), (rate, cutoff)


def test_tail_rule_and_refusals_of_the_plan(built):
    ac = ddn.FmAudioConfig(post_downsample=3)
    assert plan(ac, 0, 1024, 1024 + 2, 0, 0)[0] == ddn.DDN_ERANGE            # a tail block of 2 < M
    assert b"post_downsample" in ddn.lib().ddn_last_error()
    assert plan(ac, 0, 1024, 1024 + 3, 0, 0)[:2] == (0, 342)
    assert plan(ac, 1, 1024, 1024 + 4, 0, 0)[0] == ddn.DDN_ERANGE            # 2 after one half-band stage
    assert plan(ac, 0, 2, 64, 0, 0)[0] == ddn.DDN_ERANGE                     # every block shorter than M
    assert plan(ac, 2, 1024, 1022, 0, 0)[0] == ddn.DDN_ERANGE                # n no multiple of 2^passes
    assert plan(ac, 0, 1024, 64, 3, 0)[0] == ddn.DDN_EINVAL                  # a phase the decimator cannot be in
    assert plan(ac, -1, 1024, 64, 0, 0)[0] == ddn.DDN_EINVAL and plan(ac, 0, 0, 64, 0, 0)[0] == ddn.DDN_EINVAL
    rc, cnt, ph, ix = plan(ac, 0, 1024, 1024 + 2, 2, 0)                      # refused: the phases stay
    assert rc == ddn.DDN_ERANGE and (ph, ix) == (2, 0)


@pytest.mark.parametrize("passes", fm_audio.PASSES)
@pytest.mark.parametrize("M", fm_audio.DECIMS)
def test_counts_follow_the_restatement(built, passes, M):
    """n = 1 ... 300 (times 2^passes) as consecutive calls of one stream, under every low_pass_real setting: the plan's count and phases
    equal the restatement's at every call; calls whose tail is shorter than M are refused and leave the stream where it was"""
    zeros = np.full((300 << passes, 2), 128, np.uint8)
    for lpr in fm_audio.LPRS:
        c = fm_audio.cfg(passes=passes, M=M, lpr=lpr)
        ac = ddn.FmAudioConfig(post_downsample=M, lpr_fast_hz=lpr[0] if lpr else 0, lpr_slow_hz=lpr[1] if lpr else 0)
        rs = fm_audio.Restatement(c, block_len=256)
        ph, ix, refused = 0, 0, 0
        for k in range(1, 301):
            n = k << passes
            rc, cnt, ph2, ix2 = plan(ac, passes, 256, n, ph, ix)
            tail = k % (256 >> passes)
            if tail and tail < M:
                assert rc == ddn.DDN_ERANGE, (lpr, k)
                refused += 1
                continue
            assert rc == 0
            got = rs.run(zeros[:n])
            assert (cnt, (ph2 if M > 1 else 0, ix2 if lpr else 0)) == (len(got), rs.phases()), (lpr, k)
            ph, ix = ph2, ix2
        assert refused == (0 if M == 1 else len([k for k in range(1, 301) if 0 < k % (256 >> passes) < M]))
