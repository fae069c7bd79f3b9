"""GPU: the CQPSK demodulator kernels (ddn_cqpsk.hip, ddn_ted.hip behind ddn_cqpsk_run) at their edges against the CPU oracle, which
tests/test_oracle_cqpsk_edge.py pins bit for bit to the compiled reference on these very inputs (same rows, families and call plan:
tests/cqpsk_edge.py, which also says which FLL / LPF / Gardner kernel a row launches).

37 channels = two full 16-channel FLL workgroups and a ragged one inside a ragged 64-lane wave of the symbol-rate kernels; channel c
carries family c % 12 with seed c (12-23 negated, 24-36 with I and Q swapped), so the four lanes of a quad's neighbours hold unrelated
levels.  After every call counts and symbols equal the oracle's on the uint32 view; the eight state words equal after each of the
calls shorter than two chunks and at the end.  Nothing here is meant to fault: every family is finite input with finite results."""
import ctypes as C

import numpy as np
import pytest

import cqpsk_edge as ce
import ddn
import orc

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_calls(x, rate, sym_rate, lpf, plan, blk, **kw):
    """one channel -> (symbols of every call, state after every call)"""
    fe = orc.OracleCqpskFe(rate=rate, sym_rate=sym_rate, lpf_enable=lpf, **kw)
    pos, syms, states = 0, [], []
    for L in plan:
        syms.append(fe.run(x[pos:pos + L], blk))
        states.append(fe.state())
        pos += L
    return syms, states


def drive(b, dev_in, want, plan, watched, label, families=True):
    """dev_in [B][n][2]: the stream as the batch takes it; want[c] = oracle_calls() of channel c"""
    B, pos = dev_in.shape[0], 0
    for k, L in enumerate(plan):
        sym, cnt = b.run(dev_in[:, pos:pos + L])
        pos += L
        for c in range(B):
            where = "%s call %d (%d samples) channel %d%s" % (label, k, L, c, " (%s)" % ce.FAMILIES[c % 12] if families else "")
            w = want[c][0][k]
            assert cnt[c] == len(w), (where, int(cnt[c]), len(w))
            assert np.array_equal(u32(sym[c, :cnt[c]]), u32(w)), (where, np.flatnonzero(u32(sym[c, :cnt[c]]) != u32(w))[:4])
            if k < watched or k == len(plan) - 1:
                got = b.state(c)
                assert np.array_equal(u32(got), u32(want[c][1][k])), (where, got, want[c][1][k])


def edge_case(B, rate, sym_rate, lpf):
    sps, blk = rate // sym_rate, ce.block_len(rate)
    iq = np.stack([ce.channel_stream(c, sps, ce.n_symbols(sps)) for c in range(B)])
    plan = ce.call_plan(iq.shape[1], sps, blk, ce.lpf_taps(rate, lpf))
    want = [oracle_calls(iq[c], rate, sym_rate, lpf, plan, blk) for c in range(B)]
    b = ddn.CqpskBatch(B, rate=rate, sym_rate=sym_rate, lpf_enable=lpf, block_len=blk)
    drive(b, iq, want, plan, ce.watched_calls(sps), "%d/%d lpf %d" % (rate, sym_rate, lpf))


@pytest.mark.parametrize("row", ce.ROWS, ids=ce.row_id)
def test_rows_match_oracle(built, row):
    edge_case(37, *row[:3])


def test_generic_fll_over_nine_workgroups(built):
    """130 channels at sps 6: k_cqpsk_agc_fll<0> over nine workgroups (the last with two channels), a third, ragged wave of
    k_cqpsk_symbols, nine k_gardner_ring workgroups; the 81-tap generic LPF in front"""
    edge_case(130, 28800, 4800, 1)


@pytest.mark.parametrize("rate", [14400, 28800])
def test_cu8_input_through_the_generic_lpf(built, rate):
    """k_channel_lpf_c2c<cu8> (41 and 81 taps) does the widening; the oracle gets the widened floats"""
    B, sps, blk = 8, rate // 4800, 333
    iqf = orc.synth_dqpsk_f32(91 + sps, B, 700, sps, amp=0.5)
    u8 = np.clip(np.rint(127.5 + 127.5 * iqf), 0, 255).astype(np.uint8)
    wid = ((u8.astype(np.float32) - 127.5) * np.float32(1.0 / 127.5)).astype(np.float32)
    plan = ce.call_plan(u8.shape[1], sps, blk, ce.lpf_taps(rate, 1))
    want = [oracle_calls(wid[c], rate, 4800, 1, plan, blk) for c in range(B)]
    b = ddn.CqpskBatch(B, rate=rate, block_len=blk, input_format=ddn.IN_CU8)
    drive(b, u8, want, plan, ce.watched_calls(sps), "%d cu8" % rate, families=False)


@pytest.mark.parametrize("rate,sym_rate,held_rate,switches", ce.NONINT_ROWS)
def test_sample_rate_no_multiple_of_symbol_rate(built, rate, sym_rate, held_rate, switches):
    """the Gardner stage's gain goes by (rate + sps / 2) / sps (12000 / 4800 -> 6000, 28000 / 4800 -> 5600: the 0.018 gain once
    locked; 26000 / 4800 -> 5200: not), not by the configured symbol rate; `held` is the same sps at a rate that divides"""
    B, sps, blk = 5, rate // sym_rate, 333
    iq = orc.synth_dqpsk_f32(0, B, 900, sps)
    plan = ce.call_plan(iq.shape[1], sps, blk, 0)
    want = [oracle_calls(iq[c], rate, sym_rate, 0, plan, blk) for c in range(B)]
    held = np.concatenate(oracle_calls(iq[0], held_rate, sym_rate, 0, plan, blk)[0])
    assert np.array_equal(u32(np.concatenate(want[0][0])), u32(held)) != switches
    b = ddn.CqpskBatch(B, rate=rate, sym_rate=sym_rate, lpf_enable=0, block_len=blk)
    drive(b, iq, want, plan, ce.watched_calls(sps), "%d/%d" % (rate, sym_rate), families=False)


def test_rejected_lengths_leave_the_batch_untouched(built):
    """a call that would hand the reference's Gardner stage a block of 1-3 samples is refused with DDN_ERANGE before anything runs:
    the next legal call equals an oracle that never saw the refused ones"""
    B, rate, sps, blk = 5, 24000, 5, 333
    iq = np.stack([ce.channel_stream(c + 5, sps, 300) for c in range(B)])
    b = ddn.CqpskBatch(B, rate=rate, lpf_enable=1, block_len=blk)
    fes = [orc.OracleCqpskFe(rate=rate, lpf_enable=1) for _ in range(B)]
    pos = 0
    for L, legal in [(700, True), (3, False), (blk + 2, False), (77, True), (2 * blk + 1, False), (blk + 4, True)]:
        part = np.ascontiguousarray(iq[:, pos:pos + L])
        stride = ddn.lib().ddn_cqpsk_max_symbols(b.h, L)
        sym = np.zeros((B, stride), np.float32)
        cnt = np.zeros(B, np.int32)
        rc = ddn.lib().ddn_cqpsk_run_host(b.h, part.ctypes.data, L, sym.ctypes.data, stride, cnt.ctypes.data)
        if not legal:
            assert rc == ddn.DDN_ERANGE, (L, rc)
            continue
        assert rc == ddn.DDN_OK, (L, rc)
        pos += L
        for c in range(B):
            w = fes[c].run(part[c], blk)
            assert cnt[c] == len(w) and np.array_equal(u32(sym[c, :cnt[c]]), u32(w)), (L, c)
            assert np.array_equal(u32(b.state(c)), u32(fes[c].state())), (L, c)


def test_lpf_that_needs_more_taps_than_the_cap_is_refused(built):
    """96 kHz with the channel LPF: the design asks for 269 taps, the cap is 143 (the reference falls back to a fixed table there, which
    this build does not carry) -> DDN_ERANGE, no batch"""
    cfg = ddn.CqpskConfig(4, 96000, 4800, 5, 1, ddn.IN_CF32, 1000, 0.0)
    h = C.c_void_p()
    assert ddn.lib().ddn_cqpsk_batch_create(C.byref(cfg), C.byref(h)) == ddn.DDN_ERANGE
    assert not h.value
