"""GPU: differential fuzz of ddn_cq_rx (dsd-neo_amd/csrc/ddn_cqrx.hip, the symbol-rate receive loop of both CQPSK chains) against
orc.OracleCqRx, channel by channel and call by call: the 10-byte records, flags and counts, the events (position, kind, a, b, data4),
and ddn_cq_rx_get_state.  Where the loop's per-symbol path can go wrong: batches of 1 - 200 channels, both protocols and lock modes,
the SNR weight, the five dibit maps under either polarity, exact levels (ties) to heavy noise, DC offsets, gains of 1e-3 - 1e3, streams
long enough for the 1024-deep extrema rings to wrap several times, ragged call splits (the carried window extrema restart every call),
counts of 0 and 1, a call with nothing in it, the edge streams of tests/cqrx_edge.py (NaN, infinities, signed zeros, denormals, huge
magnitudes) among clean channels, full event buffers, row strides wider than the call, d_counts_in = NULL and a reset mid-stream.
DDN_FUZZ_BASE shifts the seeds."""
import ctypes as C
import os

import numpy as np
import pytest

import cqrx_edge
import ddn
import orc
from test_cqrx_gpu import INV, LEVEL, p1_traffic

pytestmark = pytest.mark.gpu

FZ = 7919 * int(os.environ.get("DDN_FUZZ_BASE", "0"))
INV = {**INV, 1: {c: r for r, c in enumerate([2, 3, 0, 1])}}   # + the reverse map (never a sync map: hunts only)
P2_SYNC = np.array([int(c) for c in "11131131111333133333"])


def levels(dibits, rng, map_idx, invert, noise, offset, gain):
    d = np.asarray(dibits, np.int64) ^ (2 if invert else 0)
    raw = np.vectorize(INV[map_idx].get)(d)
    return ((LEVEL[raw].astype(np.float64) + noise * rng.standard_normal(len(d))) * gain + offset).astype(np.float32)


def p2_train(rng, n):
    parts = [rng.integers(0, 4, int(rng.integers(0, 60)))]
    while sum(len(p) for p in parts) < n:
        parts += [P2_SYNC, rng.integers(0, 4, 700), rng.integers(0, 4, int(rng.integers(0, 30)))]
    return np.concatenate(parts)[:n]


_POOL = {}


def p1_pool(k):
    """a few P25 Phase 1 traffic dibit streams (control, voice, data), made once: channels take rotated slices of them"""
    if k not in _POOL:
        rng = np.random.default_rng(900 + k)
        _POOL[k] = np.concatenate([p1_traffic(rng, kind) for kind in ("ctrl", "voice", "data", "ctrl")])
    return _POOL[k]


def oracle_snr(snr):
    return -100.0 if snr == 0.0 else snr                                # (the config's 0 = not given)


class Dev:
    """ddn_cq_rx through its C API: device rows of `stride` floats (padding NaN: a read past a channel's count shows), d_counts_in
    given or NULL, the raw event count as the kernel reports it"""

    def __init__(self, B, protocol, lock, snr, max_events):
        self.B, self.E = B, max_events
        self.rx = ddn.CqRx(B, protocol, lock, snr, max_events=max_events)
        self.l = ddn.lib()

    def run(self, rows, counts, stride, null_counts=False):
        l, B = self.l, self.B
        n = max([len(r) for r in rows] + [0])
        assert stride >= n
        blk = np.full((B, max(stride, 1)), np.nan, np.float32)
        for c, r in enumerate(rows):
            blk[c, :len(r)] = r
        d = {k: C.c_void_p() for k in ("sym", "cin", "rec", "fl", "cnt")}
        for k, nb in (("sym", blk.nbytes), ("cin", B * 4), ("rec", max(B * n * 10, 4)), ("fl", max(B * n, 4)), ("cnt", B * 4)):
            assert l.ddn_device_alloc(nb, C.byref(d[k])) == 0
        assert l.ddn_device_upload(d["sym"], blk.ctypes.data, blk.nbytes) == 0
        cin = None
        if not null_counts:
            cc = np.ascontiguousarray(counts, np.int32)
            assert l.ddn_device_upload(d["cin"], cc.ctypes.data, cc.nbytes) == 0
            cin = d["cin"]
        assert l.ddn_cq_rx_run(self.rx.h, d["sym"], cin, n, stride, d["rec"], d["fl"], d["cnt"], n, None) == 0
        rec, fl, cnt = np.zeros((B, n, 10), np.uint8), np.zeros((B, n), np.uint8), np.zeros(B, np.int32)
        ev, nev, evd = np.zeros((B, self.E, 4), np.int32), np.zeros(B, np.int32), np.zeros((B, self.E, 4), np.int32)
        for a, p in ((rec, d["rec"]), (fl, d["fl"]), (cnt, d["cnt"]), (ev, self.rx.d_ev), (nev, self.rx.d_nev), (evd, self.rx.d_evd)):
            if a.nbytes:
                assert l.ddn_device_download(a.ctypes.data, p, a.nbytes) == 0
        for p in d.values():
            l.ddn_device_free(p)
        return rec, fl, cnt, ev, nev, evd

    def reset(self):
        assert self.l.ddn_cq_rx_reset(self.rx.h, None) == 0

    def close(self):
        self.rx.close()


def same_f32(got, want):
    """bitwise, but any NaN equals any NaN: the payload an operation makes is the hardware's (x86's default NaN has the sign bit set,
    the GPU's does not), not the loop's"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(nan | (got.view(np.uint32) == want.view(np.uint32))))


def check_call(tag, got, orx, x, ev_from, pos0):
    """one channel after one call: records / flags / count / events / state against the oracle that has just run `x`; pos0 = the
    oracle's symbol count before the call (the device's event positions count from the call's first record)"""
    rec, fl, cnt, ev, nev, evd, st = got
    n = len(x)
    wrec, wfl = orx.run(x)
    assert cnt == n, (tag, cnt, n)
    assert np.array_equal(fl[:n] & 0x7F, wfl), (tag, "flags", np.flatnonzero((fl[:n] & 0x7F) != wfl)[:5])
    assert np.array_equal(rec[:n, 0].astype(np.int32), wrec[:, 0]), (tag, "dibit", np.flatnonzero(rec[:n, 0] != wrec[:, 0])[:5])
    assert np.array_equal(rec[:n, 1].astype(np.int32), wrec[:, 1]), (tag, "reliability", np.flatnonzero(rec[:n, 1] != wrec[:, 1])[:5])
    llr = rec[:n, 2:6].copy().view(np.int16).reshape(n, 2).astype(np.int32)
    assert np.array_equal(llr, wrec[:, 2:4]), (tag, "llr", np.flatnonzero((llr != wrec[:, 2:4]).any(axis=1))[:5])
    assert np.array_equal(rec[:n, 6:10].copy().view(np.uint32).reshape(-1), x.view(np.uint32)), (tag, "symbol")
    # events of this call: the device keeps the first max_events and reports how many there were (ddn_cqrx.hip push_event)
    rows, data = orx.events.rows(), orx.events.data()
    want = list(zip(rows[ev_from:], data[ev_from:]))
    assert nev == len(want), (tag, "n_events", nev, len(want))
    for k in range(min(nev, ev.shape[0])):
        (wp, wk, wa, wb, wc), wd = want[k]
        # the device's b = the oracle's b (low 16 bits) | its c << 16: NID NAC | DUID, TSBK byte 1 | last / list index, MPDU end | byte 0
        wb_dev = int(np.uint32((wb & 0xFFFF) | ((wc & 0xFFFF) << 16)).view(np.int32))
        assert (int(ev[k, 0]) + pos0, ev[k, 1], ev[k, 2], ev[k, 3]) == (wp, wk, wa, wb_dev), (tag, "event", k, tuple(ev[k]), (wp, wk, wa, wb, wc))
        assert np.array_equal(evd[k], wd), (tag, "event data", k, evd[k], wd)
    # state {centre, max, min, map, last sync, in frame, hunted, extrema index}: the device keeps no centre word and reports
    # (max + min) / 2, the centre the next in-frame symbol slices around; the other seven are the oracle's own
    ws = orx.state()
    with np.errstate(invalid="ignore"):
        centre = (ws[1] + ws[2]) / np.float32(2.0)
    assert same_f32(st[1:], ws[1:]), (tag, "state", st, ws)
    assert same_f32(st[0], centre), (tag, "state centre", st, ws)


def drive(streams, protocol, lock, snr, calls, max_events=1024, stride_extra=None, null_calls=(), reset_after=None, tag="fuzz"):
    """streams: f32 per channel; calls: per call the counts (B,), summing per channel to the stream lengths.  stride_extra: {call:
    extra floats per row}; null_calls: calls run with d_counts_in = NULL (their counts all equal); reset_after: ddn_cq_rx_reset after
    that call, and the oracles start afresh.  -> syncs seen"""
    B = len(streams)
    p2 = protocol == ddn.CQ_P25P2
    mk = lambda: orc.OracleCqRx(orc.CQ_P25P2 if p2 else orc.CQ_P25P1, (lock if lock > 0 else 700) if p2 else (lock if lock > 0 else -1),
                                oracle_snr(snr))
    dev = Dev(B, protocol, lock, snr, max_events)
    orcs = [mk() for _ in range(B)]
    done, pos, sync = [0] * B, [0] * B, 0
    try:
        for ci, cnt in enumerate(calls):
            rows = [np.ascontiguousarray(streams[c][done[c]:done[c] + int(cnt[c])]) for c in range(B)]
            assert all(len(r) == int(k) for r, k in zip(rows, cnt))
            n = max([len(r) for r in rows] + [0])
            null = ci in null_calls
            assert not null or len(set(int(v) for v in cnt)) == 1
            rec, fl, co, ev, nev, evd = dev.run(rows, cnt, n + (stride_extra or {}).get(ci, 0), null)
            for c in range(B):
                ev_from = orcs[c].events.n
                check_call((tag, c, ci), (rec[c], fl[c], co[c], ev[c], nev[c], evd[c], dev.rx.state(c)), orcs[c], rows[c], ev_from, pos[c])
                sync += int(np.count_nonzero(fl[c, :len(rows[c])] & 2))
                done[c] += len(rows[c])
                pos[c] += len(rows[c])
            if reset_after == ci:
                dev.reset()
                orcs = [mk() for _ in range(B)]
                pos = [0] * B
        assert all(d == len(s) for d, s in zip(done, streams))
    finally:
        dev.close()
    return sync


def splits(rng, lengths, n_calls):
    """ragged counts per call: random cuts per channel, some forced to counts of 0 and 1, and one call with nothing in it"""
    B = len(lengths)
    cuts = np.zeros((B, n_calls + 1), np.int64)
    for c, L in enumerate(lengths):
        k = np.sort(rng.integers(0, L + 1, n_calls - 1))
        for j in range(1, len(k)):
            u = rng.random()
            if u < 0.15:
                k[j] = k[j - 1]                                            # a count of 0
            elif u < 0.3:
                k[j] = min(k[j - 1] + 1, L)                                # a count of 1
        cuts[c, 1:-1], cuts[c, -1] = k, L
    calls = [np.diff(cuts[:, j:j + 2], axis=1)[:, 0] for j in range(n_calls)]
    calls.insert(int(rng.integers(0, n_calls + 1)), np.zeros(B, np.int64))
    return calls


def make_stream(rng, protocol, L, edge=None):
    if (rng.random() < 0.8) == (protocol == ddn.CQ_P25P2):
        d = p2_train(rng, L)
    else:
        pool = p1_pool(int(rng.integers(0, 3)))
        d = np.resize(np.roll(pool, -int(rng.integers(0, len(pool)))), L)
    noise = 0.0 if rng.random() < 0.2 else float(rng.uniform(0.0, 0.6))
    gain = float(10 ** rng.uniform(-3, 3)) if rng.random() < 0.3 else 1.0
    s = levels(d, rng, int(rng.integers(0, 5)), bool(rng.integers(0, 2)), noise, float(rng.normal(0, 0.3)), gain)
    if edge is not None:
        s = cqrx_edge.edge_stream(edge, s, int(rng.integers(0, L - 400)), seed=int(rng.integers(0, 1 << 30)))
    return s


@pytest.mark.parametrize("seed", range(24))
def test_seeded_fuzz(built, seed):
    rng = np.random.default_rng(FZ + 1009 * seed + 17)
    B = int(rng.integers(1, 201))
    mode = int(rng.integers(0, 4))                                          # P1 handlers / P1 fixed count / P2 700 / P2 other count
    protocol = ddn.CQ_P25P1 if mode < 2 else ddn.CQ_P25P2
    lock = 0 if mode in (0, 2) else int(rng.integers(20, 1200))
    snr = float(rng.choice([0.0, -60.0, 3.0, 12.5, 25.0, 40.0]))
    L = int(rng.integers(3500, 4500))
    names = cqrx_edge.edge_names()
    lengths = [L - int(rng.integers(0, 300)) for _ in range(B)]
    streams = [make_stream(rng, protocol, Lc, names[int(rng.integers(0, len(names)))] if rng.random() < 0.08 else None) for Lc in lengths]
    n_calls = int(rng.integers(2, 7))
    null_calls = ()
    if rng.random() < 0.3:                                                  # a first call with d_counts_in = NULL
        u = int(rng.integers(0, min(lengths) + 1))
        calls = [np.full(B, u)] + splits(rng, [Lc - u for Lc in lengths], n_calls)
        null_calls = (0,)
    else:
        calls = splits(rng, lengths, n_calls)
    stride_extra = {int(rng.integers(0, len(calls))): int(rng.integers(1, 97))} if rng.random() < 0.4 else None
    max_events = int(rng.choice([1, 3, 1024, 1024])) if mode == 0 else 1024
    reset_after = int(rng.integers(0, len(calls) - 1)) if rng.random() < 0.25 else None
    drive(streams, protocol, lock, snr, calls, max_events, stride_extra, null_calls, reset_after, tag=("seed", seed, B, mode, lock, snr))


@pytest.mark.parametrize("protocol,lock", [(ddn.CQ_P25P2, 0), (ddn.CQ_P25P1, 900), (ddn.CQ_P25P1, 0)])
def test_edge_streams_among_clean_channels(built, protocol, lock):
    """every edge of tests/cqrx_edge.py on its own channel, written where the loop is in frame, each beside a clean channel; both
    equal the oracle, and the clean ones still lock"""
    rng = np.random.default_rng(FZ + 77 + protocol * 3 + lock)
    streams, edge_at = [], []
    for k, name in enumerate(cqrx_edge.edge_names()):
        d = p2_train(rng, 2600) if protocol == ddn.CQ_P25P2 else np.resize(np.roll(p1_pool(k % 3), -int(rng.integers(0, 5000))), 2600)
        clean = levels(d, rng, int(rng.choice([0, 2, 3, 4])), bool(k & 1), 0.25, 0.1, 1.0)
        streams += [cqrx_edge.edge_stream(name, clean, 1000 + 3 * k, seed=k), clean]
    calls = splits(rng, [len(s) for s in streams], 4)
    sync = drive(streams, protocol, lock, 12.5, calls, tag=("edge", protocol, lock))
    assert sync >= 2 * len(cqrx_edge.edge_names())


@pytest.mark.parametrize("max_events", [1, 3])
def test_event_buffer_overflow(built, max_events):
    """P25 Phase 1 control traffic with the handlers in the loop and room for 1 / 3 events a call: the device keeps the oracle's first
    events and reports the number the call produced, full buffer or not"""
    rng = np.random.default_rng(FZ + 5 + max_events)
    streams = [levels(np.resize(np.roll(p1_pool(c % 3), -int(rng.integers(0, 5000))), 3000), rng, 0, False, 0.2, 0.0, 1.0) for c in range(6)]
    calls = splits(rng, [3000] * 6, 3)
    dev = Dev(6, ddn.CQ_P25P1, 0, 0.0, max_events)
    seen = 0
    try:
        done = 0
        for cnt in [np.full(6, 1500), np.full(6, 1500)]:
            rec, fl, co, ev, nev, evd = dev.run([s[done:done + 1500] for s in streams], cnt, 1500)
            seen = max(seen, int(nev.max()))
            done += 1500
    finally:
        dev.close()
    assert seen > max_events                                                # (the buffer did overflow)
    drive(streams, ddn.CQ_P25P1, 0, 0.0, calls, max_events=max_events, tag=("overflow", max_events))


def test_direct_api_stride_null_counts_and_reset(built):
    """ddn_cq_rx_run with rows wider than the call and d_counts_in = NULL, then ddn_cq_rx_reset mid-stream: equal to fresh oracles"""
    rng = np.random.default_rng(FZ + 4242)
    for protocol, lock in ((ddn.CQ_P25P2, 0), (ddn.CQ_P25P1, 0)):
        streams = [make_stream(rng, protocol, 3600) for _ in range(7)]
        calls = [np.full(7, 1100), np.full(7, 0), np.full(7, 1), np.full(7, 999)] + splits(rng, [1500] * 7, 2)
        drive(streams, protocol, lock, 3.0, calls, stride_extra={0: 13, 2: 64, 3: 1}, null_calls=(0, 1, 2, 3), reset_after=2,
              tag=("api", protocol))
