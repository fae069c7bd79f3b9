"""CPU: the CQPSK chain restatement (oracle/ddn_oracle_cqpsk.c) pinned bit for bit against full_demod(cqpsk_enable) of the compiled
reference on exactly the inputs the device test (tests/test_cqpsk_edge_gpu.py) compares the kernels with: every row of
cqpsk_edge.ROWS, every signal family, handed over call by call under cqpsk_edge.call_plan with one reference handle kept across the
calls.  Symbols and the eight state words equal after every call.

Each family also has to show, on the reference's own result, that it reached the edge it is named for (the witnesses below): an input
that stays in the middle of the number format proves nothing about its ends.

What test_rows_match_reference prints (run with -s) on the reference's results, seed 0: the share of the silence_then_signal stream's
last 200 symbols within 0.5 of +-1 / +-3 (symbols spread evenly over (-4, 4) score 0.5; LOCK_FLOOR lies halfway to 1; from sps 8 up the
streams are 1500 symbols long, cqpsk_edge.n_symbols: at 700 the loops are not locked there, 0.51 - 0.72), and the final |fll_freq| of the
three carrier-offset families.  FLL_FLOOR is half of the smallest |fll_freq| of a family that is not dropped (0.0141); cfo_pi cannot meet
a floor from sps 4 up and is dropped there by name in cqpsk_edge.ROWS.

  9600-4800-lpf0   sps  2  lock 1.00  cfo_pi 0.1070  cfo_neg 0.1275  cfo1 0.0907
  9600-4800-lpf1   sps  2  lock 1.00  cfo_pi 0.1071  cfo_neg 0.1322  cfo1 0.1090
  14400-4800-lpf0  sps  3  lock 1.00  cfo_pi 0.0556  cfo_neg 0.0594  cfo1 0.0518
  14400-4800-lpf1  sps  3  lock 1.00  cfo_pi 0.0556  cfo_neg 0.0594  cfo1 0.0532
  24000-6000-lpf0  sps  4  lock 1.00  cfo_pi 0.0010  cfo_neg 0.0459  cfo1 0.0388
  24000-6000-lpf1  sps  4  lock 1.00  cfo_pi 0.0025  cfo_neg 0.0459  cfo1 0.0445
  24000-4800-lpf0  sps  5  lock 1.00  cfo_pi 0.0000  cfo_neg 0.0373  cfo1 0.0307
  24000-4800-lpf1  sps  5  lock 1.00  cfo_pi 0.0012  cfo_neg 0.0373  cfo1 0.0333
  28800-4800-lpf0  sps  6  lock 1.00  cfo_pi 0.0001  cfo_neg 0.0315  cfo1 0.0261
  28800-4800-lpf1  sps  6  lock 1.00  cfo_pi 0.0011  cfo_neg 0.0315  cfo1 0.0290
  38400-4800-lpf1  sps  8  lock 1.00  cfo_pi 0.0008  cfo_neg 0.0501  cfo1 0.0477
  48000-6000-lpf1  sps  8  lock 1.00  cfo_pi 0.0008  cfo_neg 0.0501  cfo1 0.0513
  48000-4800-lpf1  sps 10  lock 1.00  cfo_pi 0.0003  cfo_neg 0.0404  cfo1 0.0391
  96000-4800-lpf0  sps 20  lock 1.00  cfo_pi 0.0001  cfo_neg 0.0206  cfo1 0.0171
  115200-4800-lpf0 sps 24  lock 1.00  cfo_pi 0.0001  cfo_neg 0.0174  cfo1 0.0144
  120000-4800-lpf0 sps 25  lock 1.00  cfo_pi 0.0001  cfo_neg 0.0170  cfo1 0.0141
"""
import numpy as np
import pytest

import cqpsk_edge as ce
import orc

needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="compiled reference (oracle/_ref) not present")

FLL_FLOOR = 0.007
LOCK_FLOOR = 0.75
SUBNORMAL_MAX = np.float32(2.0 ** -126)


def run_both(x, rate, sym_rate, lpf, plan, blk):
    """-> the reference's symbols per call and its final state, after asserting the oracle equal call by call"""
    ref = orc.RefCqpskFe(rate=rate, sym_rate=sym_rate, lpf_enable=lpf)
    fe = orc.OracleCqpskFe(rate=rate, sym_rate=sym_rate, lpf_enable=lpf)
    pos, out = 0, []
    for k, L in enumerate(plan):
        w, g = ref.run(x[pos:pos + L], blk), fe.run(x[pos:pos + L], blk)
        pos += L
        assert len(w) == len(g), (k, L, len(w), len(g))
        assert np.array_equal(w.view(np.uint32), g.view(np.uint32)), (k, L, np.flatnonzero(w.view(np.uint32) != g.view(np.uint32))[:4])
        ws, gs = ref.state(), fe.state()
        assert np.array_equal(ws.view(np.uint32), gs.view(np.uint32)), (k, L, ws, gs)
        out.append(w)
    st = ref.state()
    ref.close()
    return out, st


def near_levels(sym):
    return np.minimum(np.abs(np.abs(sym) - 1.0), np.abs(np.abs(sym) - 3.0)) < 0.5


def witness(name, sym, st, dropped=()):
    assert np.isfinite(sym).all(), name                       # every family is finite input for which the reference is finite
    if name == "subnormal":
        assert 0.0 < st[0] < SUBNORMAL_MAX, st[0]
    elif name == "overflow":
        assert st[0] == np.inf and len(sym) > 200 and not sym[64:].any(), st[0]
    elif name == "silence_then_signal":
        z = np.flatnonzero(sym[:400] == 0.0)
        longest = max(np.split(z, np.flatnonzero(np.diff(z) != 1) + 1), key=len)
        assert len(longest) >= 100, len(longest)
        after = sym[longest[-1] + 1:]
        assert len(after) >= 400 and np.count_nonzero(after) >= len(after) - 2, (len(after), np.count_nonzero(after))
        assert near_levels(after[-200:]).mean() > LOCK_FLOOR, near_levels(after[-200:]).mean()     # spread evenly over (-4, 4): 0.5
    elif name in ce.CFO and name not in dropped:
        assert abs(st[1]) > FLL_FLOOR, (name, st[1])


@needs_ref
@pytest.mark.parametrize("row", ce.ROWS, ids=ce.row_id)
def test_rows_match_reference(built, row):
    rate, sym_rate, lpf, dropped = row
    sps, blk = rate // sym_rate, ce.block_len(rate)
    line = []
    for name in ce.FAMILIES:
        x = ce.family(name, sps, ce.n_symbols(sps))
        plan = ce.call_plan(len(x), sps, blk, ce.lpf_taps(rate, lpf))
        out, st = run_both(x, rate, sym_rate, lpf, plan, blk)
        if name in ce.CFO:
            line.append("%s %.4f" % (name, abs(st[1])))
        if name == "silence_then_signal":
            line.append("lock %.2f" % near_levels(np.concatenate(out)[-200:]).mean())
        witness(name, np.concatenate(out), st, dropped)
    print("%-16s sps %2d  %s" % (ce.row_id(row), sps, "  ".join(line)))


@needs_ref
@pytest.mark.parametrize("rate,sym_rate,held_rate,switches", ce.NONINT_ROWS)
def test_sample_rate_no_multiple_of_symbol_rate(built, rate, sym_rate, held_rate, switches):
    """the Gardner gain goes by (rate + sps / 2) / sps: 12000 / 4800 is sps 2 at 6000 sym/s, 28000 / 4800 sps 5 at 5600 - the 0.018
    side of the 5500 threshold once 240 symbols have locked - and 26000 / 4800 sps 5 at 5200, which stays at 0.025.  The held run is
    the same sps at a rate that divides (derived rate 4800: the gain never switches; without the LPF nothing else sees the rate)."""
    sps, blk = rate // sym_rate, 333
    x = orc.synth_dqpsk_f32(0, 1, 900, sps)[0]
    plan = ce.call_plan(len(x), sps, blk, 0)
    out, _ = run_both(x, rate, sym_rate, 0, plan, blk)
    sym = np.concatenate(out)
    held = orc.OracleCqpskFe(rate=held_rate, sym_rate=sym_rate, lpf_enable=0)
    pos, parts = 0, []
    for L in plan:
        parts.append(held.run(x[pos:pos + L], blk))
        pos += L
    held = np.concatenate(parts)
    assert len(sym) == len(held) > 800
    same = np.array_equal(sym.view(np.uint32), held.view(np.uint32))
    assert same != switches
    if switches:
        assert np.array_equal(sym[:240].view(np.uint32), held[:240].view(np.uint32))      # the switch needs 240 locked symbols
    assert near_levels(sym[-300:]).mean() > 0.9


def test_call_plan_holds_its_promises():
    for sps, blk, taps in [(2, 333, 27), (4, 333, 0), (5, 333, 67), (6, 333, 81), (10, 1000, 135), (24, 1000, 0)]:
        n = ce.n_symbols(sps) * sps - 40
        plan = ce.call_plan(n, sps, blk, taps)
        NT = ce.fll_taps(sps)
        TS = 3 * NT if NT in ce.REG_NT else 32
        assert n - 3 <= sum(plan) <= n and ce.watched_calls(sps) == 12 + NT
        assert plan[:12] == [4, 5, 6, 7] * 3
        assert sorted(plan[12:12 + NT]) == list(range(NT, 2 * NT))
        assert plan[12 + NT:18 + NT] == [TS - 1, TS, TS + 1, 2 * TS, 2 * TS + 1, 3 * TS + 1]
        if taps:
            assert plan[18 + NT:21 + NT] == [blk + 4, blk + taps - 1, blk + taps]
    with pytest.raises(AssertionError):
        ce.call_plan(700 * 5 - 40, 5, 30, 0)          # 11 + 20 = 31 samples would leave a 1-sample block: refused, not adjusted
