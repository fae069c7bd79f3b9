"""GPU: the analog FM monitor (ddn_batch_set_audio_monitor -> ddn_fm_audio_run, k_fm_audio behind the channel LPF) against the CPU
restatement of full_demod()'s audio output kind (tests/fm_audio_ref.c, pinned to the compiled reference by test_fm_audio_oracle.py) and
against the compiled reference's recorded outputs (tests/golden/fm_audio_*.npz).  Every comparison is bit for bit: samples, counts and
the carried state of ddn_batch_get_audio_state."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import ddn
import fm_audio
from fm_audio import BLOCK, OCCO, bits, cfg

pytestmark = pytest.mark.gpu


def check(c, iq, calls=None, what=None):
    got, gst = fm_audio.device_batch(ddn, c, iq, calls)
    want, wst = fm_audio.restate_batch(c, iq, calls)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (what, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(bits(gst), bits(wst)), (what, gst[0], wst[0])
    return got


def nearest(n, p):
    return max(1 << p, int(round(n / float(1 << p))) << p)


@functools.lru_cache(maxsize=None)
def lengths_case(passes):
    """130 channels through calls of 1, 63, 64, 65 and 4001 samples (the nearest multiples of 2^passes): ragged tiles, a short last block;
    restated once, shared by the channel counts"""
    c = cfg(passes=passes, lpf=3000, lpr=(48000, 32000))
    calls = [nearest(n, passes) for n in (1, 63, 64, 65, 4001)]
    iq = fm_audio.synth_nfm(11 + passes, 130, sum(calls))
    rs = [fm_audio.Restatement(c) for _ in range(130)]
    parts, pos = [], 0
    for m in calls:
        parts.append(np.stack([r.run(iq[ch, pos:pos + m]) for ch, r in enumerate(rs)]))
        pos += m
    return c, calls, iq, parts, np.stack([r.state() for r in rs])


@pytest.mark.parametrize("passes", fm_audio.PASSES)
@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_channels_and_lengths(built, B, passes):
    """1 / 63 channels: a partial wavefront; 65: a second workgroup with one live lane; 130: a third with two"""
    c, calls, iq, want, wst = lengths_case(passes)
    b = fm_audio.make_batch(ddn, c, B, ddn.IN_CU8)
    pos = 0
    for k, m in enumerate(calls):
        assert b.max_samples(m) >= want[k].shape[1]
        got = b.run_host(np.ascontiguousarray(iq[:B, pos:pos + m]), m)
        assert got.shape == (B, want[k].shape[1]), (k, got.shape, want[k].shape)
        assert np.array_equal(bits(got), bits(want[k][:B])), (k, m, np.argwhere(bits(got) != bits(want[k][:B]))[:4])
        pos += m
    st = np.stack([b.audio_state(ch) for ch in range(B)])
    assert np.array_equal(bits(st), bits(wst[:B]))


@pytest.mark.parametrize("passes", fm_audio.PASSES)
@pytest.mark.parametrize("M", fm_audio.DECIMS)
def test_polyphase_decimator_across_twenty_short_calls(built, M, passes):
    k = 7 << passes
    iq = fm_audio.synth_nfm(7, 3, 20 * k)
    check(cfg(passes=passes, M=M, lpr=(48000, 32000)), iq, [k] * 20, (M, passes))


@pytest.mark.parametrize("lpr", fm_audio.LPRS)
def test_low_pass_real(built, lpr):
    iq = fm_audio.synth_nfm(21, 2, 5001)
    for M in (1, 3):
        check(cfg(lpr=lpr, M=M), iq, [4001, 1000], (lpr, M))


@pytest.mark.parametrize("name", [n for n in sorted(fm_audio.configs()) if n.startswith(("sw_", "tau"))])
def test_filter_switches(built, name):
    check(fm_audio.configs()[name], fm_audio.synth_nfm(31, 2, 2000), None, name)


@pytest.mark.parametrize("name", ["squelch_above", "squelch_below", "squelch_mid", "squelch_mid_env"])
def test_squelch_levels(built, name):
    got = check(fm_audio.configs()[name], fm_audio.synth_nfm(41, 3, 4096, amp_blocks=OCCO), None, name)
    if name == "squelch_above":
        assert not got.any()


def test_squelch_open_closed_closed_open(built):
    """one block per call: the envelope's values, zeros while closed, and the first sample behind the closed run - an atan2f of signed
    zeros, +-pi where the first open sample lies in the third quadrant (re = -0)"""
    c = cfg(squelch=0.02, deemph=0, dc=0)
    B = 12
    iq = fm_audio.synth_nfm(51, B, 4 * BLOCK, amp_blocks=OCCO)
    b = fm_audio.make_batch(ddn, c, B, ddn.IN_CU8)
    rs = [fm_audio.Restatement(c) for _ in range(B)]
    envs = []
    for k in range(4):
        part = np.ascontiguousarray(iq[:, k * BLOCK:(k + 1) * BLOCK])
        got = b.run_host(part, BLOCK)
        want = np.stack([r.run(part[ch]) for ch, r in enumerate(rs)])
        assert np.array_equal(bits(got), bits(want)), k
        st = np.stack([b.audio_state(ch) for ch in range(B)])
        assert np.array_equal(bits(st), bits(np.stack([r.state() for r in rs]))), k
        envs.append(st[:, 6].tolist())
        if k in (1, 2):
            # closed: zeros out (but the block's first sample: a phase step from the last open sample to 0 + 0j, an atan2f of signed
            # zeros as well), pre_r / pre_j zero
            assert not got[:, 1:].any() and not st[:, 7].any() and not st[:, :2].any()
        if k == 3:
            first = got[:, 0] / np.float32(st[0, 6])
            assert np.any(np.abs(first) > 3.1), first                                 # atan2f(+-0, -0) = +-pi in some channel
            assert np.all((np.abs(first) > 3.1) | (first == 0)), first                # ... and +-0 in the others
    assert envs == [[1.0] * B, [0.96875] * B, [0.9384765625] * B, [0.9461669921875] * B]


def test_call_splitting(built):
    """6 blocks in one call == 6 calls of one block == calls of 2 + 3 + 1 blocks, states included"""
    c = cfg(squelch=0.02, M=3, lpr=(48000, 32000), lpf=3000)
    iq = fm_audio.synth_nfm(61, 5, 6 * BLOCK, amp_blocks=[0.6, 0.04, 0.6, 0.6, 0.04, 0.6])
    one = check(c, iq, None)
    for calls in ([BLOCK] * 6, [2 * BLOCK, 3 * BLOCK, BLOCK]):
        got, st = fm_audio.device_batch(ddn, c, iq, calls)
        assert np.array_equal(bits(got), bits(one))
        assert np.array_equal(bits(st), bits(fm_audio.restate_batch(c, iq)[1]))


@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
def test_input_formats_agree_on_the_widened_data(built, fmt):
    c = cfg(M=2, passes=1)
    iq = fm_audio.synth_nfm(71, 3, 3000, fmt=fmt)
    a = check(c, iq)
    b = check(c, fm_audio.widen(iq))
    assert np.array_equal(bits(a), bits(b))


def test_non_finite_samples_propagate_as_in_the_restatement(built):
    c = cfg(M=2, lpr=(48000, 32000), squelch=0.001)
    iq = fm_audio.widen(fm_audio.synth_nfm(81, 2, 3000)).copy()
    iq[0, 700, 0] = np.nan
    iq[1, 1500, 1] = np.inf
    got, gst = fm_audio.device_batch(ddn, c, iq)
    want, wst = fm_audio.restate_batch(c, iq)
    assert np.isnan(want).any()
    assert fm_audio.same_bits(got, want) and fm_audio.same_bits(gst, wst)


def test_mode_checks_and_refusals(built):
    l = ddn.lib()
    B, n = 2, 512
    iq = fm_audio.synth_nfm(91, B, n)
    out = np.full((B, n), 7.0, np.float32)
    cnt = C.c_size_t(99)
    au = fm_audio.make_batch(ddn, cfg(M=3), B, ddn.IN_CU8, block_len=256)
    assert l.ddn_front_end_run_host(au.h, iq.ctypes.data, n, out.ctypes.data) == ddn.DDN_EINVAL
    assert b"audio-monitor" in l.ddn_last_error() and (out == 7.0).all()
    assert l.ddn_batch_set_iq_conditioning(au.h, 1, 11, 0, 0.0, 0.0) == ddn.DDN_EINVAL and b"IQ conditioning" in l.ddn_last_error()
    seg = np.array([1, 1], np.int32)
    prof = np.array([0, 0], np.int32)
    assert l.ddn_batch_set_segments(au.h, 2, seg.ctypes.data, prof.ctypes.data) == ddn.DDN_EINVAL and b"segment" in l.ddn_last_error()
    # the tail rule: 256 + 2 leaves a block of 2 < 3; nothing runs, the stream stays where it was
    assert l.ddn_fm_audio_host_run(au.h, iq.ctypes.data, 258, out.ctypes.data, n, C.byref(cnt)) == ddn.DDN_ERANGE
    assert cnt.value == 0 and (out == 7.0).all()
    # a row too short for the call's count
    assert l.ddn_fm_audio_host_run(au.h, iq.ctypes.data, 300, out.ctypes.data, 99, C.byref(cnt)) == ddn.DDN_ERANGE and (out == 7.0).all()
    assert au.max_samples(300) == 100
    got = au.run_host(iq[:, :300], 300)
    assert np.array_equal(bits(got), bits(fm_audio.restate_batch(cfg(M=3), iq[:, :300], block_len=256)[0]))
    # a decimator longer than a block, and the mode against a batch that has IQ conditioning set
    plain = ddn.Batch(B, lpf_profile=ddn.LPF_WIDE, block_len=256)
    assert l.ddn_batch_set_audio_monitor(plain.h, C.byref(ddn.FmAudioConfig(post_downsample=300))) == ddn.DDN_ERANGE
    assert l.ddn_fm_audio_host_run(plain.h, iq.ctypes.data, n, out.ctypes.data, n, C.byref(cnt)) == ddn.DDN_EINVAL
    assert b"not set to the audio-monitor kind" in l.ddn_last_error() and (out == 7.0).all()
    assert l.ddn_fm_audio_max_samples(plain.h, n) == 0
    plain.set_iq_conditioning(1, 11, 0, 0.0, 0.0)
    assert l.ddn_batch_set_audio_monitor(plain.h, C.byref(ddn.FmAudioConfig())) == ddn.DDN_EINVAL and b"IQ conditioning" in l.ddn_last_error()
    # reset: a fresh stream, the integer phases included
    au.reset()
    assert np.array_equal(bits(au.run_host(iq[:, :300], 300)), bits(got))
    # and back to the FSK kind: the batch's discriminator route as before
    assert l.ddn_batch_set_audio_monitor(au.h, None) == 0
    ref = ddn.Batch(B, lpf_profile=ddn.LPF_WIDE, block_len=256)
    assert np.array_equal(bits(ddn.Batch.run_host(au, iq, n)), bits(ref.run_host(iq, n)))


def test_adapter_full_demod_audio_monitor(built):
    """full_demod() with output_kind 0 on a fresh demod_state: the restatement's result_len and samples, block by block"""
    l = ddn.lib()
    c = cfg(passes=1, M=2, lpr=(96000, 48000), lpf=3000, squelch=0.02)
    c3, _ = fm_audio.Restatement(c).coefficients()
    iq = fm_audio.widen(fm_audio.synth_nfm(95, 1, 3 * BLOCK, amp_blocks=[0.6, 0.04, 0.6])[0]).copy()
    s = ddn.DemodState()
    s.rate_in, s.rate_out, s.output_kind = 96000, 48000, 0
    s.channel_lpf_enable, s.channel_lpf_profile, s.channel_squelch_level = 1, ddn.LPF_WIDE, 0.02
    s.downsample_passes, s.post_downsample, s.deemph, s.deemph_a = 1, 2, 1, float(c3[0])
    s.audio_lpf_enable, s.audio_lpf_alpha, s.dc_block, s.rate_out2 = 1, float(c3[1]), 1, 48000
    s.squelch_env, s.squelch_gate_open = 1.0, 1
    rs = fm_audio.Restatement(c, block_len=1 << 16)
    for k in range(3):
        blk = np.ascontiguousarray(iq[k * BLOCK:(k + 1) * BLOCK])
        s.lowpassed = blk.ctypes.data_as(C.POINTER(C.c_float))
        s.lp_len = 2 * BLOCK
        l.full_demod(C.byref(s))
        want = rs.run(blk)
        assert s.result_len == len(want) > 0, (k, s.result_len, l.ddn_last_error())
        assert np.array_equal(bits(np.ctypeslib.as_array(s.result)[:s.result_len]), bits(want)), k
        assert (np.float32(s.squelch_env), s.squelch_gate_open) == (rs.state()[6], int(rs.state()[7]))
    l.ddn_demod_state_release(C.byref(s))


@pytest.mark.parametrize("name", sorted(fm_audio.GOLDEN))
def test_device_equals_golden(built, name):
    g = np.load(fm_audio.golden_path(name))
    c = json.loads(str(g["cfg_json"]))
    c["lpr"] = tuple(c["lpr"]) if c["lpr"] else None
    got, st = fm_audio.device_batch(ddn, c, g["iq"], [int(m) for m in g["calls"]])
    assert got.shape == g["audio"].shape and np.array_equal(bits(got), bits(g["audio"]))
    assert np.array_equal(bits(st), bits(g["state"]))
    b = fm_audio.make_batch(ddn, c, 1, ddn.IN_CU8)
    assert np.array_equal(bits(b.coefficients()[1]), bits(g["taps"]))


def test_decode_capture_tool_writes_the_analog_wav(built, tmp_path):
    """tools/decode_capture.py CAPTURE --analog OUT.wav: the restatement's samples (de-emphasis, DC block, low_pass_real to 8 kHz) as 16-bit
    PCM at full scale pi"""
    import os
    import sys
    import wave
    import cs16
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import decode_capture
    iq = fm_audio.synth_nfm(97, 1, 20000)[0]
    path = cs16.write_capture(str(tmp_path / "nfm_cu8.iq"), iq, "cu8")
    lines = []
    pcm = decode_capture.decode_analog(path, str(tmp_path / "out.wav"), out=lines.append)
    want = fm_audio.Restatement(cfg(lpr=(48000, 8000)), block_len=8192).run(iq)
    assert np.array_equal(bits(pcm), bits(want)) and "8000 Hz" in lines[0]
    with wave.open(str(tmp_path / "out.wav")) as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (8000, 1, 2, len(want))
        s16 = np.frombuffer(w.readframes(len(want)), np.int16)
    assert np.abs(s16.astype(np.float64) - want.astype(np.float64) / np.pi * 32767.0).max() <= 1.0


def reachable_count_table(c, longest):
    """the restatement's output count after 0 .. longest samples (behind the half-band stages) of a fresh stream, each length one
    block of its own run, and the period after which the two carried integers (decimator phase, low_pass_real index) repeat"""
    p, M = c["passes"], c["M"]
    zeros = np.full((longest << p, 2), 128, np.uint8)
    counts = [0]
    for k in range(1, longest + 1):
        try:
            counts.append(len(fm_audio.Restatement(c, block_len=1 << 14).run(zeros[:k << p])))
        except ValueError:                       # shorter than M from a fresh phase: no decimator output yet
            assert k < M
            counts.append(0)
    fast, slow = c["lpr"] if c["lpr"] else (1, 1)
    return counts, M * (fast // np.gcd(fast, slow))


@pytest.mark.parametrize("passes", fm_audio.PASSES)
@pytest.mark.parametrize("M", fm_audio.DECIMS)
def test_max_samples_is_the_tight_bound_over_every_carried_phase(built, M, passes):
    """ddn_fm_audio_max_samples(n) for n = 1 ... 300 (times 2^passes) under every low_pass_real setting: at least the restatement's count
    from every reachable (decimator phase, low_pass_real index) start, and equal to the largest of them.  A start is reached by the
    samples of one period of the two integers; the count from it is a difference of the fresh stream's running count."""
    for lpr in fm_audio.LPRS:
        c = cfg(passes=passes, M=M, lpr=lpr)
        counts, period = reachable_count_table(c, 300 + 30)
        assert period <= 30
        b = fm_audio.make_batch(ddn, c, 1, ddn.IN_CU8)
        for k in range(1, 301):
            from_starts = [counts[o + k] - counts[o] for o in range(period)]
            assert b.max_samples(k << passes) == max(from_starts), (lpr, k, from_starts)
        b.close()


def test_decimation_set_on_an_audio_batch_starts_a_fresh_stream(built):
    """ddn_batch_set_decimation on a batch already in the audio kind resets it, the two integer phases included"""
    c = cfg(M=3, lpr=(48000, 32000))
    iq = fm_audio.synth_nfm(98, 2, 2048)
    b = fm_audio.make_batch(ddn, c, 2, ddn.IN_CU8)
    b.run_host(iq[:, :1000], 1000)                      # leaves both phases off zero
    b.set_decimation(1)
    got = b.run_host(iq, 2048)
    want, wst = fm_audio.restate_batch(cfg(M=3, lpr=(48000, 32000), passes=1), iq)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(np.stack([b.audio_state(ch) for ch in range(2)])), bits(wst))


@pytest.mark.parametrize("block_len", [136, 150, 200])
def test_block_lengths_that_are_no_multiple_of_the_tile(built, block_len):
    """every block ends in a ragged tile (a batch takes no block shorter than the channel LPF's 135 taps, so 136 is the shortest)"""
    c = cfg(M=3, lpr=(48000, 32000), squelch=0.02, lpf=3000)
    iq = fm_audio.synth_nfm(99, 3, 7 * block_len + 50, amp_blocks=[0.6, 0.04, 0.6, 0.04, 0.04, 0.6], block_len=block_len)
    got, gst = fm_audio.device_batch(ddn, c, iq, [3 * block_len, 4 * block_len + 50], block_len=block_len)
    want, wst = fm_audio.restate_batch(c, iq, [3 * block_len, 4 * block_len + 50], block_len=block_len)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(gst), bits(wst))


def test_host_variant_checks_its_arguments_before_it_touches_the_device(built):
    """what test_cabi_exports.py's table checks for the symbols ending in _host, for ddn_fm_audio_host_run on a live batch: a null
    buffer or count is DDN_EINVAL with the call's name, nothing is written and the stream stays where it was"""
    l = ddn.lib()
    iq = fm_audio.synth_nfm(93, 1, 512)
    out = np.full((1, 512), 7.0, np.float32)
    cnt = C.c_size_t(5)
    b = fm_audio.make_batch(ddn, cfg(), 1, ddn.IN_CU8)
    for args in ((None, 512, out.ctypes.data, 512, C.byref(cnt)), (iq.ctypes.data, 512, None, 512, C.byref(cnt)),
                 (iq.ctypes.data, 512, out.ctypes.data, 512, None)):
        assert l.ddn_fm_audio_host_run(b.h, *args) == ddn.DDN_EINVAL and b"ddn_fm_audio_host_run" in l.ddn_last_error()
    assert l.ddn_fm_audio_run(b.h, None, 512, out.ctypes.data, 512, C.byref(cnt), None) == ddn.DDN_EINVAL
    assert (out == 7.0).all() and cnt.value == 5
    assert l.ddn_fm_audio_host_run(b.h, iq.ctypes.data, 0, out.ctypes.data, 512, C.byref(cnt)) == 0 and cnt.value == 0
    assert np.array_equal(bits(b.run_host(iq, 512)), bits(fm_audio.restate_batch(cfg(), iq)[0]))
