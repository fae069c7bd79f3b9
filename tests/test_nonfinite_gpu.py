"""Non-finite input must stay contained: NaN / Inf samples in some channels neither hang a kernel (every data-dependent
loop is bounded) nor leak into the other channels of the batch, which still equal the oracle bit for bit."""
import numpy as np
import pytest

import ddn
import orc

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_front_end_and_rx_with_nan_inf_channels(built):
    B, n = 20, 12000
    iq8 = orc.synth_c4fm_cu8(50, B, n)
    iq = ((iq8.astype(np.float32) - 127.5) / 127.5).astype(np.float32)
    bad = [3, 7, 16]
    iq[3, 1000:1100] = np.nan
    iq[7, 5000:5003, 0] = np.inf
    iq[16, ::97, 1] = -np.inf
    fe = ddn.Batch(B, input_format=ddn.IN_CF32, block_len=4096)
    disc = fe.run_host(iq, n)
    for c in range(B):
        if c in bad:
            continue
        want = orc.OracleFrontEnd().run_f32(iq[c], 4096)
        assert np.array_equal(bits(disc[c]), bits(want)), c
    rx = ddn.P25Rx(B, lock_symbols=840, use_matched_filter=1)
    x, _, _ = orc.synth_p25_disc(3, B, n, frame_dibits=432)
    x[2, 3000:3050] = np.nan
    x[9, 7000] = np.inf
    x[11] = np.nan                                           # a channel that is NaN throughout
    rec, fl, cnt = rx.run(x)
    for c in range(B):
        if c in (2, 9, 11):
            assert 0 < cnt[c] <= rec.shape[1]
            continue
        o = orc.OracleP25Rx(lock_symbols=840, use_filter=1)
        sym, rec4, flo = o.run(x[c])
        k = int(cnt[c])
        r4, sy = orc.unpack_records10(rec[c, :k])
        assert k == len(sym) and np.array_equal(sy.view(np.uint32), sym.view(np.uint32)) and np.array_equal(r4, rec4), c


def test_gardner_and_cqpsk_with_nan_inf_channels(built):
    import ctypes as C
    B, sps = 12, 5
    iq = orc.synth_dqpsk_f32(5, B, 1200, sps)
    n = iq.shape[1]
    iq[1, 400:420] = np.nan                                  # the timing loop zeroes NaN components like the reference
    iq[4, 2000, 0] = np.inf                                  # Inf is not sanitised: that channel's loop state goes non-finite
    iq[6] = np.inf
    b = ddn.CqpskBatch(B, rate=24000, block_len=2048)
    sym, cnt = b.run(iq)
    for c in range(B):
        if c in (1, 4, 6):
            assert 0 <= cnt[c] <= sym.shape[1]
            continue
        want = orc.OracleCqpskFe(rate=24000).run(iq[c], 2048)
        assert cnt[c] == len(want) and np.array_equal(bits(sym[c, :cnt[c]]), bits(want)), c


FSK4 = ["dmr", "nxdn48", "nxdn96", "m17", "ysf", "dpmr", "dstar", "edacs"]


@pytest.mark.parametrize("name", FSK4)
def test_fsk4_loop_with_a_nan_inf_channel(built, name):
    """every protocol of the fsk4 receive loop: channel 2 of five carries NaN, +Inf and -Inf runs inside a capture slice; the call
    returns, every count stays within its bound, and the channels on both sides of it - lanes of the same wavefront - equal the oracle
    bit for bit, in the call that holds the runs and in the one after it"""
    import fuzz_rx4 as fz
    import rx4
    from test_rx4_gpu import check_channel
    B, n = 5, 24000
    if name in fz.ROWS:
        row, s = fz.ROWS[name], fz.scan(name)
        disc, at = s["disc"], int(s["sync_at"][0])
        proto, sps, win = row.gpu_proto, 48000 // row.sym_rate, row.win_len
        oracle = lambda: row.oracle(row.rf_mod0, 48000, row.default_lock())
        rf_mod = row.rf_mod0
    else:
        cap, lpf, p, proto, sps, win = (("iq_dmr_t3_ras_cc.npz", 2, rx4.PROTO_DMR, ddn.FSK4_DMR, 10, 24) if name == "dmr" else
                                        ("iq_nxdn48.npz", 1, rx4.PROTO_NXDN48, ddn.FSK4_NXDN48, 20, 10))
        disc, at, rf_mod = rx4.capture_disc(cap, lpf), 61000, 0
        oracle = lambda: rx4.OracleFsk4Rx(rx4.profile(p))
    at = max(0, min(at - 1500, len(disc) - n - 200))
    x = np.stack([disc[at + 37 * c:at + 37 * c + n] for c in range(B)]).astype(np.float32)
    x[3] = -x[3]
    x[2, 3000:3050] = np.nan
    x[2, 7000] = np.inf
    x[2, 9000:9040] = -np.inf
    x[2, 9500:9600:7] = np.inf
    gpu = ddn.Fsk4Rx(B, proto, rf_mod=rf_mod)
    assert ddn.lib().ddn_fsk4_rx_set_channels_per_wave(gpu.h, 8) == 0       # (all five in one wavefront)
    cpu = [oracle() for _ in range(B)]
    n_sync = 0
    for a, b in ((0, 12001), (12001, n)):
        got = gpu.run_host(x[:, a:b])                                        # (raises unless the call returns 0)
        ms, my = got["rec"].shape[1], got["sync_pos"].shape[1]
        assert (ms, my) == (fz.max_symbols(b - a, sps), fz.max_syncs(b - a, sps, win))
        assert (got["cnt"] >= 0).all() and (got["cnt"] <= ms).all() and (got["n_sync"] >= 0).all() and (got["n_sync"] <= my).all()
        assert 0 < got["cnt"][2] <= ms
        for c in (0, 1, 3, 4):
            want = cpu[c].run(x[c, a:b], max_sync=my)
            check_channel(got, c, want)
            assert np.array_equal(bits(gpu.thresholds(c)), bits(cpu[c].thresholds())), c
            n_sync += len(want["sync_pos"])
    gpu.close()
    assert n_sync >= 4
