"""cs16 input on the FSK front end: the fused kernel's cs16 instances, the half-band cascade's and the channel-LPF route's, against
the CPU oracle's f32 entry on widen(x) and against a cf32 batch on widen(x).

Bar: bit for bit, no tolerance anywhere - the widening float(s) * 2^-15 is exact (tests/cs16.py), so a cs16 run and a cf32 run on the
widened samples do the same arithmetic on the same floats.  Every stream carries the extreme pairs (cs16.SALT) in a first tile, in
a prefetched tile, in the look-back of every call and across a block edge."""
import numpy as np
import pytest

import cs16
import ddn
import orc

pytestmark = pytest.mark.gpu


def same(got, want, what=None):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = got.view(np.uint32) != want.view(np.uint32)
    assert not ne.any(), (what, np.argwhere(ne)[:5])


def run_calls(batch, x, calls):
    out, lo = [], 0
    for n in calls:
        out.append(batch.run_host(np.ascontiguousarray(x[:, lo:lo + n]), n))
        lo += n
    return np.concatenate(out, axis=1)


def oracle_calls(w, calls, blk, **kw):
    """-> (float32 [B, total], the oracle objects) of channel-wise streaming runs with the same call boundaries"""
    rows, fes = [], []
    for c in range(w.shape[0]):
        fe = orc.OracleFrontEnd(**kw)
        lo, parts = 0, []
        for n in calls:
            parts.append(fe.run_f32(np.ascontiguousarray(w[c, lo:lo + n]), blk))
            lo += n
        rows.append(np.concatenate(parts))
        fes.append(fe)
    return np.stack(rows), fes


def both(B, x, calls, blk, prepare=None, **kw):
    """the cs16 batch on x and the cf32 batch on widen(x), call for call"""
    w = cs16.widen(x)
    res = []
    for fmt, data in ((ddn.IN_CS16, x), (ddn.IN_CF32, w)):
        b = ddn.Batch(B, block_len=blk, input_format=fmt, **kw)
        if prepare:
            prepare(b)
        res.append((run_calls(b, data, calls), b))
    return res[0], res[1], w


@pytest.mark.parametrize("blk,n", [(2048, 6000), (3000, 9001), (135, 1000), (257, 7 * 257 + 33)])
def test_block_sizes_and_ragged_tails(built, blk, n):
    B = 5
    x = cs16.synth_c4fm_cs16(3, B, n, blk)
    (got, _), (cf, _), w = both(B, x, [n], blk)
    same(got, cf, "cf32 batch")
    same(got, oracle_calls(w, [n], blk)[0], "oracle")
    assert (got[:, 0] == 0.0).all()


def test_calls_carry_state_and_a_call_shorter_than_the_look_back(built):
    """two long calls, then 50 samples (fewer than the DDN_CARRY_LEN = 72 of look-back: the carry kernel shifts history and widens
    the new samples itself), then a call that filters across that history; the modem state equals the oracle's; reset() repeats"""
    B, blk = 5, 4096
    calls = [3 * blk, 2 * blk + 777, 50, 1500]
    total = sum(calls)
    x = cs16.synth_c4fm_cs16(11, B, total, blk, calls=calls)
    x[:, calls[0] + calls[1] + 20:calls[0] + calls[1] + 26] = cs16.SALT          # inside the 50-sample call
    (got, b), (cf, bf), w = both(B, x, calls, blk)
    want, fes = oracle_calls(w, calls, blk)
    same(got, cf, "cf32 batch")
    same(got, want, "oracle")
    for c in range(B):
        st = np.asarray(b.fsk_state(c), np.float32)[:5]
        assert np.array_equal(st.view(np.uint32), cs16.oracle_fsk_state(fes[c]).view(np.uint32)), (c, st)
        assert np.array_equal(st.view(np.uint32), np.asarray(bf.fsk_state(c), np.float32)[:5].view(np.uint32)), c
    b.reset()
    again = b.run_host(np.ascontiguousarray(x[:, :calls[0]]), calls[0])
    same(again, got[:, :calls[0]], "after reset")


@pytest.mark.parametrize("B,n,blk", [(9, 3000, 1024), (2064, 700, 256)])
def test_both_workgroup_shapes(built, B, n, blk):
    """8 channels per workgroup with the second workgroup holding one channel; above 2048 channels 16 per workgroup (129 workgroups)"""
    x = cs16.synth_c4fm_cs16(100, B, n, blk)
    (got, _), (cf, _), w = both(B, x, [n], blk)
    same(got, cf, "cf32 batch")
    same(got, oracle_calls(w, [n], blk)[0], "oracle")


@pytest.mark.parametrize("rate,profile,taps", [(48000, 4, 135), (24000, 1, 67), (32000, 2, 89)])
def test_tap_length_instances(built, rate, profile, taps):
    """the unrolled centre-67 and centre-33 instances and the run-time one.  SKIPZ: the unrolled instances are launched with it only
    when a designed tap is zero, which no rate / profile pair gives (so through the library they run as SKIPZ = false, here too);
    the run-time instance is always launched as SKIPZ = true."""
    B, blk, calls = 3, 4096, [5000, 4001]
    x = cs16.synth_c4fm_cs16(41, B, sum(calls), blk, calls=calls)
    (got, b), (cf, _), w = both(B, x, calls, blk, sample_rate_hz=rate, lpf_profile=profile)
    assert len(b.taps()) == taps
    same(got, cf, "cf32 batch")
    same(got, oracle_calls(w, calls, blk, rate=rate, profile=profile)[0], "oracle")


@pytest.mark.parametrize("blk", [2048, 256])
def test_squelch_gate(built, blk):
    """quiet blocks are int16 zeros (the cs16 zero is exact, unlike cu8's 127 / 128); one-tile blocks take the alternating halves"""
    B = 4
    calls = [5 * blk, 3 * blk + 33]
    n = sum(calls)
    x = cs16.synth_c4fm_cs16(31, B, n, blk, calls=calls)
    for c in range(B):
        x[c, 2 * blk + 17 * c:4 * blk + 9 * c] = 0
    x[1, 6 * blk:7 * blk] = 0
    (got, _), (cf, _), w = both(B, x, calls, blk, squelch_level=0.01)
    want = oracle_calls(w, calls, blk, squelch=0.01)[0]
    assert (want[:, 3 * blk:4 * blk] == 0).all() and (want[:, :blk] != 0).any()
    same(got, cf, "cf32 batch")
    same(got, want, "oracle")


@pytest.mark.parametrize("passes", [1, 2])
def test_halfband_cascade(built, passes):
    """input at 96 / 192 kHz: cs16 enters the 31-tap first stage (k_hb_decim2 / k_hb_hist), the cascade goes on in cf32"""
    B, blk = 3, 2048
    calls = [8192, 5120]                                                # the second call ends in half a block
    x = cs16.synth_c4fm_cs16(40, B, sum(calls), blk, calls=calls, sps=10 << passes)
    (got, _), (cf, _), w = both(B, x, calls, blk, prepare=lambda b: b.set_decimation(passes))
    want = oracle_calls(w, calls, blk, downsample_passes=passes)[0]
    assert got.shape[1] == sum(calls) >> passes
    same(got, cf, "cf32 batch")
    same(got, want, "oracle")


@pytest.mark.parametrize("rate,profile,taps", [(48000, 4, 135), (24000, 1, 67), (32000, 2, 89)])
def test_iq_conditioning_route(built, rate, profile, taps):
    """dc blocker + IQ balance on: the unfused route, whose first kernel is k_channel_lpf_c2c (unrolled 135- and 67-tap forms and
    the generic one) with k_lpf_hist carrying its history"""
    B, blk, calls = 3, 2048, [6000, 3001]
    x = cs16.synth_c4fm_cs16(51, B, sum(calls), blk, calls=calls)
    prep = lambda b: b.set_iq_conditioning(dc_enable=1, dc_shift=11, bal_enable=1)
    (got, b), (cf, _), w = both(B, x, calls, blk, prepare=prep, sample_rate_hz=rate, lpf_profile=profile)
    assert len(b.taps()) == taps
    same(got, cf, "cf32 batch")
    rows = []
    for c in range(B):
        fe = orc.OracleFrontEnd(rate=rate, profile=profile).set_iq_options(dc_enable=1, dc_shift=11, bal_enable=1)
        rows.append(np.concatenate([fe.run_f32(np.ascontiguousarray(w[c, :calls[0]]), blk),
                                    fe.run_f32(np.ascontiguousarray(w[c, calls[0]:]), blk)]))
    same(got, np.stack(rows), "oracle")


def test_misaligned_device_pointer_is_refused(built):
    import torch
    B, n = 2, 1000
    d = torch.zeros(B * n * 2 + 8, dtype=torch.int16, device="cuda:0")
    out = torch.zeros((B, n), dtype=torch.float32, device="cuda:0")
    b = ddn.Batch(B, block_len=512, input_format=ddn.IN_CS16)
    assert d.data_ptr() % 4 == 0
    rc = ddn.lib().ddn_front_end_run(b.h, d.data_ptr() + 2, n, out.data_ptr(), None)
    assert rc == ddn.DDN_EINVAL and b"aligned" in ddn.lib().ddn_last_error()
    assert ddn.lib().ddn_front_end_run(b.h, d.data_ptr() + 4, n, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
