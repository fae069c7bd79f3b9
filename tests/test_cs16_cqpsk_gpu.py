"""cs16 input on the CQPSK front end: k_channel_lpf_c2c's cs16 instances (the unrolled 135- and 67-tap forms and the generic one) and
k_lpf_hist's, ahead of the unchanged AGC / FLL / Gardner / Costas stages.  Symbols and counts equal, bit for bit, the cf32 batch on
widen(x) and the CPU oracle's f32 entry on the same floats (the widening is exact, tests/cs16.py)."""
import numpy as np
import pytest

import cs16
import ddn
import orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rate,sps,form", [(24000, 5, 67), (48000, 10, 135), (19200, 4, 0)])
def test_cqpsk_batch_cs16(built, rate, sps, form):
    B, blk = 4, 2048
    taps = np.zeros(144, np.float32)
    nt = orc.oracle().orc_channel_lpf_design(rate, ddn.LPF_P25_CQPSK, taps.ctypes.data, 144)
    assert nt == form if form else nt not in (67, 135) and nt >= 3          # which kernel form this rate reaches
    n_sym = 1500
    n1 = 2 * blk + 300
    x = cs16.synth_dqpsk_cs16(7, B, n_sym, sps, blk)
    n = x.shape[1]
    n2 = n - n1                                                            # ragged: no multiple of the block
    assert n2 > 1000 and n2 % blk >= 4
    x = cs16.salt(x, cs16.salt_positions(n, blk, calls=[n1, n2]))
    w = cs16.widen(x)
    res = []
    for fmt, data in ((ddn.IN_CS16, x), (ddn.IN_CF32, w)):
        b = ddn.CqpskBatch(B, rate=rate, sym_rate=4800, input_format=fmt, block_len=blk)
        res.append([b.run(np.ascontiguousarray(data[:, :n1])), b.run(np.ascontiguousarray(data[:, n1:])), b])
    for k in range(2):
        (sg, cg), (sf, cf) = res[0][k], res[1][k]
        assert np.array_equal(cg, cf) and int(cg.min()) > (n1, n2)[k] // (sps + 1)
        assert np.array_equal(sg.view(np.uint32), sf.view(np.uint32)), k
    for c in range(B):
        fe = orc.OracleCqpskFe(rate=rate, sym_rate=4800, profile=ddn.LPF_P25_CQPSK, lpf_enable=1)
        for k, (lo, hi) in enumerate(((0, n1), (n1, n))):
            want = fe.run(np.ascontiguousarray(w[c, lo:hi]), blk)
            sg, cg = res[0][k]
            assert int(cg[c]) == len(want), (c, k)
            assert np.array_equal(sg[c, :len(want)].view(np.uint32), want.view(np.uint32)), (c, k)
        assert np.array_equal(res[0][2].state(c).view(np.uint32), fe.state().view(np.uint32)), c


def test_cs16_without_the_channel_lpf_is_refused(built):
    """the channel LPF stage does the widening: a cs16 (like a cu8) batch without it has nothing to run on"""
    b = ddn.CqpskBatch(2, rate=24000, lpf_enable=0, input_format=ddn.IN_CS16, block_len=1024)
    with pytest.raises(ddn.DdnError, match="rc=-1 .*cs16"):
        b.run(np.zeros((2, 2048, 2), np.int16))
