"""CPU: the restatement of full_demod()'s audio-monitor kind (tests/fm_audio_ref.c) against the COMPILED REFERENCE (oracle/_ref, driven by
tests/fm_audio_refdrv.cpp), bit for bit: samples, counts, carried state, the integer phases and the decimator's taps, on every
configuration the GPU tests walk.  Skips only where the reference's sources or oracle/_ref are absent."""
import numpy as np
import pytest

import fm_audio
from fm_audio import bits

pytestmark = pytest.mark.skipif(not fm_audio.have_reference(), reason="no compiled reference on this machine")

CONFIGS = fm_audio.configs()


def both(c, iq, calls):
    rs, rf = fm_audio.Restatement(c), fm_audio.Reference(c)
    pos = 0
    for m in calls:
        a, b = rs.run(iq[pos:pos + m]), rf.run(iq[pos:pos + m])
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (pos, m, a.shape, b.shape)
        pos += m
    assert np.array_equal(bits(rs.state()), bits(rf.state())), (rs.state(), rf.state())
    assert rs.phases() == rf.phases()
    return rs, rf


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_restatement_equals_reference(built, name):
    c = CONFIGS[name]
    n = 4000                                         # three full blocks and a ragged one, a multiple of 4
    for ch, fmt in enumerate(("cu8", "cs16")):
        iq = fm_audio.synth_nfm(40 + ch, 1, n, fmt=fmt, amp_blocks=fm_audio.OCCO)[0]
        rs, rf = both(c, iq, [n])
        if c["M"] > 1:
            assert np.array_equal(bits(rs.coefficients()[1]), bits(rf.taps()))
        both(c, iq, [1024, 2048, 928])               # call boundaries on block boundaries: the same stream in three calls


@pytest.mark.parametrize("passes", fm_audio.PASSES)
@pytest.mark.parametrize("M", fm_audio.DECIMS)
def test_twenty_short_calls_wrap_ring_and_phase(built, passes, M):
    k = 7 << passes
    iq = fm_audio.synth_nfm(7, 1, 20 * k)[0]
    both(fm_audio.cfg(passes=passes, M=M, lpr=(48000, 32000)), iq, [k] * 20)


def test_squelch_envelope_and_signed_zero_restart(built):
    """blocks open, closed, closed, open: the envelope's values, zeros while closed, and the first sample after the closed run, an atan2f
    of signed zeros (cf32 input whose first open sample makes re = -0)"""
    c = fm_audio.cfg(squelch=0.02, deemph=0, dc=0)
    iq = fm_audio.widen(fm_audio.synth_nfm(3, 1, 4096, amp_blocks=fm_audio.OCCO)[0]).copy()
    rs = fm_audio.Restatement(c)
    out = rs.run(iq)
    assert not out[1024:3072].any() and out[:1024].any()
    rs2 = fm_audio.Restatement(c)
    envs = []
    for k in range(4):
        rs2.run(iq[1024 * k:1024 * (k + 1)])
        envs.append(float(rs2.state()[6]))
    assert envs == [1.0, 0.96875, 0.9384765625, 0.946166992187500]
    both(c, iq, [4096])
