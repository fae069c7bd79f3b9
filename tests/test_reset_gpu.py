"""GPU: a reset object equals a fresh one.  One scheme for every object of the C ABI that has a reset: two unrelated streams X and Y;
object A runs X, is reset and runs Y in two calls; object B, created and configured like A, runs the same two calls of Y.  A and B
agree bit for bit on every output, count and readable state, and both agree with a fresh CPU oracle fed the same calls of Y.

Premise of every case: right after X, A differs from a fresh object - in its readable state where the object has a getter for it,
in what it makes of the first call of Y where it has none (a third object that runs X and is NOT reset) - so a reset that did
nothing fails the case.  X is scaled by 0.4, of the opposite polarity where the object has one, and ends inside a frame with a
sync held, so that nothing carried sits at its reset value.

What a setter configured before X survives the reset (per-channel lock lengths, handlers, channels per wave, armed event buffers,
the Gardner block length, the vocoder's first talk path and tail rule); carried state does not."""
import ctypes as C

import numpy as np
import pytest

import ddn
import mbe
import orc
import reset_cases as rc
from test_mbe_gpu import GpuVocoder
from test_resampler_gpu import GpuResampler
from test_rx4_gpu import check_channel
from test_slicer_gpu import GpuSlicer
from test_ted_gpu import GpuTed

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def stream():
    """a non-default HIP stream (kept alive by the caller) -> (torch stream, its handle)"""
    import torch
    s = torch.cuda.Stream()
    return s, s.cuda_stream


# ---- ddn_ted_batch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sps", [5, 25])                # k_gardner_ring / the classic delay-line kernel
def test_ted_batch_reset(built, sps):
    l = ddn.lib()
    B, n_sym, rate, blk = 70, 300, 6000, 100            # 6000 symbols/s: the loop gain is chosen per block, so block_len shows
    x = orc.synth_qpsk_f32(11 + sps, B, n_sym, sps, noise=0.08) * np.float32(0.4)
    y = orc.synth_qpsk_f32(23 + sps, B, n_sym, sps, noise=0.05)
    n = y.shape[1]
    cuts = [(0, n // 3), (n // 3, n)]
    a, b = GpuTed(B, sps, rate), GpuTed(B, sps, rate)
    for t in (a, b):
        assert l.ddn_ted_batch_set_block_len(t.h, blk) == 0
    fresh = [b.state(c) for c in range(B)]
    a.run(x)
    assert all(not same(a.state(c), fresh[c]) for c in range(B))                      # premise
    _s, st = stream()
    assert l.ddn_ted_batch_reset(a.h, st) == 0
    _s.synchronize()                                    # (the host-buffer calls below run on the null stream)
    assert all(same(a.state(c), fresh[c]) for c in range(B))
    ga = [a.run(y[:, lo:hi]) for lo, hi in cuts]
    gb = [b.run(y[:, lo:hi]) for lo, hi in cuts]
    per_call = 0
    for c in range(B):
        o, o2 = orc.OracleTed(sps, rate), orc.OracleTed(sps, rate)
        for k, (lo, hi) in enumerate(cuts):
            want = np.concatenate([o.block(y[c, p:min(p + blk, hi)]) for p in range(lo, hi, blk)])
            assert same(ga[k][c], gb[k][c]) and same(gb[k][c], want), (c, k)
            whole = o2.block(y[c, lo:hi])
            per_call += len(whole) != len(want) or not same(whole, want)
        assert same(a.state(c), b.state(c)), c
    assert per_call > 0                                 # block_len survived the reset: per-call gain selection would differ


# ---- ddn_slicer_batch ----------------------------------------------------------------------------------------------------------------
def _slicer_oracle(sym, negative):
    """-> records int32 [B][n][4], thresholds after every symbol float32 [B][n][5]"""
    o = orc.oracle()
    o.orc_slicer_init.argtypes = [C.c_void_p, C.c_int]
    o.orc_slicer_run.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    B, n = sym.shape
    rec, thr = np.zeros((B, n, 4), np.int32), np.zeros((B, n, 5), np.float32)
    for c in range(B):
        st = C.create_string_buffer(20000)
        o.orc_slicer_init(st, negative)
        o.orc_slicer_run(st, np.ascontiguousarray(sym[c]).ctypes.data, n, rec[c].ctypes.data, thr[c].ctypes.data)
    return rec, thr


@pytest.mark.parametrize("n", [100, 600])               # the sequential kernel / the parallel path (n >= 256)
def test_slicer_batch_reset(built, n):
    l = ddn.lib()
    B, neg = 70, 1
    x = np.stack([-orc.synth_c4fm_symbols(500 + c, 2 * n, scale=0.4 + 0.01 * c, noise=400) for c in range(B)])
    y = np.stack([orc.synth_c4fm_symbols(700 + c, 2 * n, scale=0.8 + 0.01 * c, noise=500) for c in range(B)])
    a, b = GpuSlicer(B, neg), GpuSlicer(B, neg)
    fresh = [b.thresholds(c) for c in range(B)]
    a.run(x)
    a.filt(x)
    assert all(not same(a.thresholds(c), fresh[c]) for c in range(B))                 # premise
    assert l.ddn_slicer_batch_reset(a.h) == 0
    assert all(same(a.thresholds(c), fresh[c]) for c in range(B))
    want, thr = _slicer_oracle(y, neg)
    wf = orc.oracle_p25_filter(y)
    for k, (lo, hi) in enumerate(((0, n), (n, 2 * n))):
        ra, rb = a.run(y[:, lo:hi]), b.run(y[:, lo:hi])
        assert np.array_equal(ra, rb), k
        assert np.array_equal(orc.unpack_records10(ra)[0], want[:, lo:hi]), k
        fa, fb = a.filt(y[:, lo:hi]), b.filt(y[:, lo:hi])
        assert same(fa, fb) and same(fa, wf[:, lo:hi]), k
        for c in range(B):
            assert same(a.thresholds(c), b.thresholds(c)) and same(a.thresholds(c), thr[c, hi - 1]), (c, k)


# ---- ddn_resampler -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M", [(3, 5), (8, 1)])
def test_resampler_reset(built, L, M):
    l = ddn.lib()
    B, nx, ny, cut = 9, 1001, 900, 333
    rng = np.random.default_rng(10 * L + M)
    x = (rng.normal(0, 9000, (B, nx)) * 0.4).astype(np.float32)
    y = (rng.normal(0, 9000, (B, ny)) + 12000 * np.sin(np.arange(ny) * 0.07)).astype(np.float32)
    a, b, kept = GpuResampler(B, L, M), GpuResampler(B, L, M), GpuResampler(B, L, M)
    a.run(x)
    kept.run(x)
    if M > 1:                                           # premise: the polyphase index is not at its reset value ...
        assert l.ddn_resampler_out_len(a.h, 7) != l.ddn_resampler_out_len(b.h, 7)
    _s, st = stream()
    assert l.ddn_resampler_reset(a.h, st) == 0
    _s.synchronize()                                    # (the host-buffer calls below run on the null stream)
    assert [l.ddn_resampler_out_len(a.h, k) for k in range(12)] == [l.ddn_resampler_out_len(b.h, k) for k in range(12)]
    stale = kept.run(y[:, :cut])
    os_ = [orc.OracleResampler(L, M) for _ in range(B)]
    for k, (lo, hi) in enumerate(((0, cut), (cut, ny))):
        ga, gb = a.run(y[:, lo:hi]), b.run(y[:, lo:hi])
        assert ga.shape == gb.shape and same(ga, gb), k
        if k == 0:                                      # ... and the 15-sample history is not either
            assert stale.shape != gb.shape or not same(stale[:, :4], gb[:, :4])
        for c in range(B):
            want = os_[c].run(y[c, lo:hi])
            assert ga.shape[1] == len(want) and same(ga[c], want), (c, k)
        assert l.ddn_resampler_out_len(a.h, 7) == l.ddn_resampler_out_len(b.h, 7)


# ---- ddn_mbe_batch -------------------------------------------------------------------------------------------------------------------
def _vocoder_oracle(codec, S, first, tail, calls):
    """the restatement over S talk paths numbered from `first` (the seed of each path's noise generator), call by call"""
    v = mbe.OracleVocoder(codec, S, tail_rule=tail)
    out = []
    for b_, r_ in calls:
        b_, r_ = np.ascontiguousarray(b_, np.uint8), np.ascontiguousarray(r_, np.int32)
        F = b_.shape[1]
        pcm, res = np.zeros((S, F, 160), np.float32), np.zeros((S, F, 5), np.int32)
        rc = mbe._o().om_process_batch(codec, C.addressof(v.tab), b_.ctypes.data, r_.ctypes.data, tail, first, S, F, pcm.ctypes.data,
                                       res.ctypes.data, C.addressof(v.cur), C.addressof(v.prev), C.addressof(v.enh))
        assert rc == 0
        out.append((pcm, res))
    return v, out


def _errors(rng, shape):
    r = np.zeros(tuple(shape) + (5,), np.int32)
    r[..., 3] = rng.choice([0, 1, 2, 4], size=shape, p=[0.6, 0.2, 0.1, 0.1])
    return r


def _finish(r):
    r[..., 1] = np.minimum(r[..., 3], 3)
    r[..., 4] = r[..., 3] - r[..., 1]
    r[..., 0] = 1
    return r


@pytest.mark.parametrize("first", [0, 1000])
@pytest.mark.parametrize("codec", [ddn.MBE_IMBE, ddn.MBE_AMBE])
def test_mbe_batch_reset(built, codec, first):
    l = ddn.lib()
    S, tail = 8, 1
    rng = np.random.default_rng(31 + codec + first)
    gen = mbe.random_imbe_bits if codec == ddn.MBE_IMBE else mbe.random_ambe_bits
    xb, yb = gen(rng, (S, 6)), gen(rng, (S, 7))
    xr, yr = np.zeros((S, 6, 5), np.int32), _errors(rng, (S, 7))
    xr[:, 3:, 3] = 7                                    # X ends in an error run: the repeat counter stands at 3
    yr[2, 1:4, 3] = 7
    if codec == ddn.MBE_IMBE:                           # a teardown frame in the second call of Y: the tail rule mutes it
        yb[5, 5] = 0
        yb[5, 5, :6] = 1                                # (prefix 0xFC, few set bits, twelve corrections)
        yr[5, 5, 3] = 12
    xr, yr = _finish(xr), _finish(yr)
    a, b = GpuVocoder(codec, S, tail_rule=tail), GpuVocoder(codec, S, tail_rule=tail)
    for g in (a, b):
        assert l.ddn_mbe_batch_set_first_stream(g.h, first, None) == 0
    _, xres = a.run(xb, xr)
    assert (xres[:, -1, 0] & 0x8).all()                 # (the last frame of X is a repeat)
    assert all(not mbe.parms_equal(p, q) for s in range(S) for p, q in zip(a.state(s), b.state(s)))      # premise
    assert a.state(0)[0].repeat != 0
    _s, st = stream()
    assert l.ddn_mbe_batch_reset(a.h, st) == 0
    _s.synchronize()
    assert all(mbe.parms_equal(p, q) for s in range(S) for p, q in zip(a.state(s), b.state(s)))
    calls = [(yb[:, :3], yr[:, :3]), (yb[:, 3:], yr[:, 3:])]
    v, want = _vocoder_oracle(codec, S, first, tail, calls)
    if codec == ddn.MBE_IMBE:                           # the tail rule set before X shows in Y (it is an IMBE rule)
        assert not np.array_equal(want[1][0], _vocoder_oracle(codec, S, first, 0, calls)[1][1][0]) and not want[1][0][5, 2].any()
    if first:                                           # the talk path's index reaches the synthesis (unvoiced noise)
        assert not np.array_equal(want[0][0], _vocoder_oracle(codec, S, 0, tail, calls)[1][0][0])
    for k, (b_, r_) in enumerate(calls):
        (pa, ra), (pb, rb) = a.run(b_, r_), b.run(b_, r_)
        assert same(pa, pb) and np.array_equal(ra, rb), k
        assert same(pa, want[k][0]) and np.array_equal(ra, want[k][1]), k
        for s in range(S):
            for p, q, w in zip(a.state(s), b.state(s), (v.cur[s], v.prev[s], v.enh[s])):
                assert mbe.parms_equal(p, q), (k, s)
            if k == 1:
                assert all(mbe.parms_equal(p, w) for p, w in zip(a.state(s), (v.cur[s], v.prev[s], v.enh[s]))), s


# ---- ddn_cqpsk_batch -----------------------------------------------------------------------------------------------------------------
def test_cqpsk_batch_reset_on_a_stream(built):
    """the reset and the next run are queued on one non-default stream with no host synchronisation in between"""
    import torch
    l = ddn.lib()
    B, sps, n_sym, blk = 12, 5, 1200, 4096
    x = orc.synth_dqpsk_f32(41, B, n_sym, sps) * np.float32(0.4)
    y = orc.synth_dqpsk_f32(43, B, n_sym, sps, cfo=-0.003)
    n = y.shape[1]
    cut = 2503
    a, b = ddn.CqpskBatch(B, block_len=blk), ddn.CqpskBatch(B, block_len=blk)
    fresh = [b.state(c) for c in range(B)]
    s, st = stream()

    def queue(obj, iq):
        d = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
        stride = l.ddn_cqpsk_max_symbols(obj.h, iq.shape[1])
        sym = torch.zeros((B, stride), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                        # (the uploads above; nothing of the object is in flight here)
        return d, sym, cnt, stride

    bufs = [queue(a, x), queue(a, y[:, :cut]), queue(a, y[:, cut:])]
    d, sym, cnt, stride = bufs[0]
    assert l.ddn_cqpsk_run(a.h, d.data_ptr(), x.shape[1], sym.data_ptr(), stride, cnt.data_ptr(), st) == 0
    assert all(not same(a.state(c), fresh[c]) for c in range(B))                      # premise (get_state synchronises)
    assert l.ddn_cqpsk_batch_reset(a.h, st) == 0
    for (d, sym, cnt, stride), (lo, hi) in zip(bufs[1:], ((0, cut), (cut, n))):
        assert l.ddn_cqpsk_run(a.h, d.data_ptr(), hi - lo, sym.data_ptr(), stride, cnt.data_ptr(), st) == 0
    s.synchronize()
    got_b = [b.run(y[:, :cut]), b.run(y[:, cut:])]
    for c in range(B):
        o = orc.OracleCqpskFe(rate=24000)
        for k, (lo, hi) in enumerate(((0, cut), (cut, n))):
            want = o.run(y[c, lo:hi], blk)
            sa, ca = bufs[1 + k][1].cpu().numpy(), bufs[1 + k][2].cpu().numpy()
            sb, cb = got_b[k]
            assert ca[c] == cb[c] == len(want), (c, k)
            assert same(sa[c, :ca[c]], sb[c, :cb[c]]) and same(sa[c, :ca[c]], want), (c, k)
        assert same(a.state(c), b.state(c)) and same(a.state(c), o.state()), c


# ---- ddn_batch in the kinds its reset was never run in ---------------------------------------------------------------------------------
BATCH_KINDS = {
    "halfband": dict(passes=2),
    "iq_conditioning": dict(iq=(1, 9, 1, 0.02, 0.2)),
    "squelch": dict(squelch=0.01),
}


@pytest.mark.parametrize("kind", sorted(BATCH_KINDS))
def test_front_end_batch_reset_on_a_stream(built, kind):
    import torch
    k_ = BATCH_KINDS[kind]
    passes, iq_opt, squelch = k_.get("passes", 0), k_.get("iq"), k_.get("squelch", 0.0)
    B, blk = 6, 1200
    nx, cuts = 5 * blk, ((0, 2 * blk + 400), (2 * blk + 400, 5 * blk + 400))
    x = orc.synth_c4fm_cu8(60, B, nx, sps=10 << passes, noise_dbc=-14.0)
    x = (127.5 + (x.astype(np.float64) - 127.5) * 0.4).round().astype(np.uint8)
    if squelch:
        x[:, 3 * blk:] = 127                            # dead air at the end of X: the last blocks are gated
    y = orc.synth_c4fm_cu8(80, B, cuts[-1][1], sps=10 << passes)

    def make():
        o = ddn.Batch(B, block_len=blk, squelch_level=squelch)
        if passes:
            o.set_decimation(passes)
        if iq_opt:
            o.set_iq_conditioning(*iq_opt)
        return o

    s, st = stream()

    def run(o, iq):
        n = iq.shape[1]
        d = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
        out = torch.full((B, n >> passes), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        o.run_device(d.data_ptr(), n, out.data_ptr(), st)
        s.synchronize()
        return out.cpu().numpy()

    a, b, kept = make(), make(), make()
    run(a, x)
    run(kept, x)
    a.reset(st)
    stale = run(kept, y[:, :cuts[0][1]])
    fes = []
    for c in range(B):
        fe = orc.OracleFrontEnd(squelch=squelch, downsample_passes=passes)
        if iq_opt:
            fe.set_iq_options(*iq_opt)
        fes.append(fe)
    for k, (lo, hi) in enumerate(cuts):
        ga, gb = run(a, y[:, lo:hi]), run(b, y[:, lo:hi])
        assert same(ga, gb), k
        if k == 0:
            assert not same(stale, gb)                  # premise: what X left behind reaches the outputs of an object not reset
        for c in range(B):
            want = fes[c].run_cu8(y[c, lo:hi], blk)
            assert len(want) == ga.shape[1] and same(ga[c], want), (c, k)
    import cs16
    for c in range(B):
        assert same(a.fsk_state(c), b.fsk_state(c)) and same(a.fsk_state(c), cs16.oracle_fsk_state(fes[c])), c


# ---- ddn_p25_rx ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cpw", [8, 64])
@pytest.mark.parametrize("handlers", [False, True])
def test_p25_rx_reset(built, handlers, cpw):
    """handlers on: the decisions are read through ddn_p25_rx_run_host_ev, and X is well-formed TSDU traffic (rc.p25_handler_x) cut
    inside a frame whose NID the handler decoded - the handlers' words and history ring have no getter, so a third object that runs
    X and is not reset shows that they reach what the loop makes of Y"""
    l = ddn.lib()
    B, n = rc.P25_B, rc.P25_N
    x, y, locks = rc.p25_case()
    if handlers:
        x = rc.p25_handler_x()

    def make():
        rx = ddn.P25Rx(B, lock_symbols=840, use_matched_filter=1, channels_per_wave=cpw, handlers=handlers, max_events=256)
        assert l.ddn_p25_rx_set_lock_symbols(rx.h, locks.ctypes.data) == 0
        return rx

    a, b, kept = make(), make(), make()
    fresh = [b.thresholds(c) for c in range(B)]
    rec, fl, cnt = a.run(x)
    assert all(fl[c, cnt[c] - 1] & 1 for c in range(B))                               # premise: X ends inside a frame ...
    if handlers:                                                                      # ... whose NID the handler decoded ...
        ev = [a.events[c, :a.n_events[c]] for c in range(B)]
        assert all(((e[:, 1] == orc.HEV_P25_NID) & (e[:, 2] > 0)).any() for e in ev)
    assert all(not same(a.thresholds(c), fresh[c]) for c in range(B))                 # ... with the slicer away from its reset values
    kept.run(x)
    stale = kept.run(y[:, :n])
    assert l.ddn_p25_rx_reset(a.h) == 0
    assert all(same(a.thresholds(c), fresh[c]) for c in range(B))
    cpu = [rc.p25_oracle(handlers, locks[c]) for c in range(B)]
    base, n_ev, syncs, events = np.zeros(B, np.int64), [0] * B, 0, 0
    for k, (lo, hi) in enumerate(((0, n), (n, 2 * n))):
        (ra, fa, ca), (rb, fb, cb) = a.run(y[:, lo:hi]), b.run(y[:, lo:hi])
        assert np.array_equal(ca, cb) and np.array_equal(ra, rb) and np.array_equal(fa, fb), k
        if k == 0:                                      # premise: without the reset every channel's first call of Y comes out otherwise
            assert all(stale[2][c] != cb[c] or not np.array_equal(stale[0][c], rb[c]) or not np.array_equal(stale[1][c], fb[c])
                       for c in range(B))
        if handlers:
            assert np.array_equal(a.n_events, b.n_events) and np.array_equal(a.events, b.events), k
            assert np.array_equal(a.event_data, b.event_data), k
        for c in range(B):
            sym, rec4, flo = cpu[c].run(y[c, lo:hi])
            kk = int(ca[c])
            r4, sy = orc.unpack_records10(ra[c, :kk])
            assert kk == len(sym) and same(sy, sym) and np.array_equal(r4, rec4) and np.array_equal(fa[c, :kk], flo), (c, k)
            assert same(a.thresholds(c), b.thresholds(c)) and same(a.thresholds(c), cpu[c].thresholds()), (c, k)
            if handlers:
                want = rc.events4(cpu[c].events.rows()[n_ev[c]:])
                data = cpu[c].events.data()[n_ev[c]:]
                n_ev[c] += len(want)
                ne = int(a.n_events[c])
                got = a.events[c, :ne].astype(np.int64)
                got[:, 0] += base[c]                    # the oracle counts symbols from its start, the device from the call's
                assert ne == len(want) and np.array_equal(got & rc.EVENT_MASK, want & rc.EVENT_MASK), (c, k, got[:4], want[:4])
                assert np.array_equal(a.event_data[c, :ne], data), (c, k)
                events += ne
            base[c] += kk
            syncs += int(np.count_nonzero(fa[c, :kk] & 2))
    assert syncs >= 2 * B and (events >= B or not handlers)                       # syncs found and decisions taken after the reset


# ---- ddn_fsk4_rx ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.FSK4_NAMES)
def test_fsk4_rx_reset(built, name):
    l = ddn.lib()
    k_ = rc.fsk4_case(name)
    B, n, x, y = rc.FSK4_B, rc.FSK4_N, k_["x"], k_["y"]
    lock4 = np.tile(np.array(k_["lock"], np.int32), (B, 1))

    def make():
        rx = ddn.Fsk4Rx(B, k_["proto"], rf_mod=k_["rf_mod"], handlers=k_["handlers"])
        assert l.ddn_fsk4_rx_set_channels_per_wave(rx.h, 8) == 0
        assert l.ddn_fsk4_rx_set_lock_symbols(rx.h, lock4.ctypes.data) == 0
        return rx

    a, b = make(), make()
    fresh = [b.thresholds(c) for c in range(B)]
    gx = a.run_host(x)
    assert all(gx["fl"][c, gx["cnt"][c] - 1] & 1 for c in range(B)) and (gx["n_sync"] > 0).all()       # premise: a sync is held
    assert all(not same(a.thresholds(c), fresh[c]) for c in range(B))
    assert l.ddn_fsk4_rx_reset(a.h) == 0
    assert all(same(a.thresholds(c), fresh[c]) for c in range(B))
    cpu = [k_["oracle"]() for _ in range(B)]
    base, n_ev, n_sync = np.zeros(B, np.int64), [0] * B, 0
    for k, (lo, hi) in enumerate(((0, n + 1), (n + 1, 2 * n))):
        ga, gb = a.run_host(y[:, lo:hi]), b.run_host(y[:, lo:hi])
        for key in ga:
            assert np.array_equal(ga[key], gb[key]), (key, k)
        for c in range(B):
            want = cpu[c].run(y[c, lo:hi], max_sync=ga["sync_pos"].shape[1])
            check_channel(ga, c, want)
            assert same(a.thresholds(c), b.thresholds(c)) and same(a.thresholds(c), cpu[c].thresholds()), (c, k)
            n_sync += len(want["sync_pos"])
            if k_["handlers"]:
                ev = rc.events4(cpu[c].events.rows()[n_ev[c]:])
                n_ev[c] += len(ev)
                got = ga["events"][c, :ga["n_events"][c]].astype(np.int64)
                got[:, 0] += base[c]
                assert len(got) == len(ev) and np.array_equal(got & rc.EVENT_MASK, ev & rc.EVENT_MASK), (c, k, got[:4], ev[:4])
            base[c] += int(ga["cnt"][c])
    assert n_sync >= 4 and (not k_["handlers"] or min(n_ev) > 0)
    a.close()
    b.close()


