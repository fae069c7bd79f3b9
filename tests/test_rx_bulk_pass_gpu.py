"""The bulk hunting pass of the receive loop with two / four channels per recurrence wave (ddn_rx.hip, handler mode): every case
bit-exact three ways - the default against every hunting symbol taken by a standard trip (ddn_p25_rx_set_debug_flags bit
1048576), against the pass taken one owner at a time (bit 4096), and some channels against the oracle: records, flags, counts,
events and event data."""
import numpy as np
import pytest

import ddn
import orc
import p25gen
from test_rx_handlers_gpu import _check, _oracle, _traffic

NAC = 0x293


def _run(x, cpw, dbg, calls=None):
    """-> (rec [B, k, 10], fl [B, k], cnt [B], events [B][ne, 4] with stream-wide symbol indices, event data [B][ne, 4]); calls: the
    stream cut into consecutive calls of these lengths (repeated) on one object"""
    B, n = x.shape
    rx = ddn.P25Rx(B, use_matched_filter=1, channels_per_wave=cpw, handlers=True, max_events=2048, debug_flags=dbg)
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + (n if calls is None else calls[(len(cuts) - 1) % len(calls)])))
    recs, fls, evs, evds = [[[] for _ in range(B)] for _ in range(4)]
    base = np.zeros(B, np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        rec, fl, cnt = rx.run(x[:, a:b])
        for c in range(B):
            recs[c].append(rec[c, :cnt[c]])
            fls[c].append(fl[c, :cnt[c]])
            e = rx.events[c, :rx.n_events[c]].astype(np.int64)
            e[:, 0] += base[c]
            evs[c].append(e)
            evds[c].append(rx.event_data[c, :rx.n_events[c]])
            base[c] += cnt[c]
    return ([np.concatenate(v) for v in recs], [np.concatenate(v) for v in fls], base.copy(), [np.concatenate(v) for v in evs],
            [np.concatenate(v) for v in evds])


def _same(a, b, what):
    for k, name in enumerate(("records", "flags", "counts", "events", "event data")):
        for c in range(len(a[0])):
            assert np.array_equal(a[k][c], b[k][c]), (what, name, c)


def _three_ways(x, cpw, oracle_channels, calls=None):
    out = _run(x, cpw, 0, calls)
    _same(out, _run(x, cpw, 1048576, calls), "every hunting symbol a standard trip")
    _same(out, _run(x, cpw, 4096, calls), "one owner at a time")
    for c in oracle_channels:
        rec, fl, ev, evd = out[0][c][None], out[1][c][None], out[3][c][None], out[4][c][None]
        _check(rec, fl, np.array([rec.shape[1]]), ev, np.array([ev.shape[1]]), 0, _oracle(x[c], 1), evd)
    return out


def _short_frames(seed, n, gap, long_every=0):
    """short frames (terminators, one-block TSDUs, undefined DUIDs) `gap` idle dibits apart, each at its own amplitude so that the
    parked max / min of a hunt differ from the limits of the hunt before; long_every: every so many frames one of 840 dibits"""
    rng = np.random.default_rng(seed)
    parts, scale = [], []
    k = 0
    while sum(len(p) for p in parts) * 10 < n:
        k += 1
        if long_every and k % long_every == 0:
            fr = p25gen.frame_with_duid(rng, NAC, 0x5, 807)
        else:
            fr = [p25gen.make_tdu(NAC), p25gen.make_frames(rng, 1, NAC, crc=True, blocks=1)[0],
                  p25gen.frame_with_duid(rng, NAC, 0x9, 40)][int(rng.integers(0, 3))]
        g = np.zeros(int(gap if np.isscalar(gap) else rng.integers(gap[0], gap[1])), np.int8)
        parts += [fr, g]
        scale += [np.full(len(fr) + len(g), [1.0, 0.7, 1.3, 0.85][k % 4])]
    return np.concatenate(parts), np.concatenate(scale)


def _mod(dib, scale, lead, noise, seed, n):
    s = p25gen.modulate_disc(dib, lead=lead, noise=noise, seed=seed, scale=scale)[:n]
    return np.concatenate([s, np.zeros(n - len(s), np.float32)])


@pytest.mark.gpu
@pytest.mark.parametrize("cpw", [4, 8])
def test_who_hunts_together(built, cpw):
    """Groups of four neighbouring channels (the lanes of one recurrence wave at eight channels per workgroup, two waves' at four):
    frames that end on the same symbol in all four (channels 0-3); the same frames staggered by 1, 5 and 12 symbols (4-7); one lane
    that hunts beside three in long frames, then two (8-11); three lanes that hunt beside one in long frames (12-15).  Every call
    starts a hunt with no history (fewer than eight symbols: the limits move inside the pass), every frame has its own amplitude,
    the gaps are 3 to 40 symbols, and the leads differ by single samples: some hundred syncs whose completing symbol falls anywhere in
    the 128-sample tile and anywhere relative to a pass (right behind one, inside one, on the tile's last symbol)."""
    B, n = 16, 24000
    x = np.zeros((B, n), np.float32)
    dib, sc = _short_frames(1, n, (3, 40))
    for c in range(4):
        x[c] = _mod(dib, sc, 203, 90.0, 50, n)
    x[3] = _mod(dib, sc, 203, 2500.0, 53, n)               # (same frames, its own noise: its slips differ)
    for c, st in zip(range(4, 8), (0, 1, 5, 12)):
        x[c] = _mod(dib, sc, 260 + 10 * st + c, [90.0, 3000.0][c % 2], 60 + c, n)
    lng, lsc = _short_frames(2, n, 2, long_every=1)
    for c in range(8, 16):
        x[c] = _mod(lng, lsc, 310 + 7 * c, 90.0, 70 + c, n)
    d2, s2 = _short_frames(3, n, (8, 30))
    x[8] = _mod(d2, s2, 231, 90.0, 78, n)
    x[9, n // 2:] = _mod(d2, s2, 337, 1500.0, 79, n)[:n - n // 2]
    for c, st in zip((12, 13, 15), (0, 3, 7)):
        x[c] = _mod(d2, s2, 222 + 10 * st + c, [90.0, 2000.0][c % 2], 90 + c, n)
    out = _three_ways(x, cpw, (0, 3, 7, 8, 9, 13))
    syncs = [int((out[1][c] & 2).sum()) for c in range(B)]
    assert min(syncs[:8]) >= 10 and min(syncs[8:]) >= 2, syncs                # frames were received: the hunts are real ones


@pytest.mark.gpu
@pytest.mark.parametrize("cpw", [4, 8])
def test_rows_and_limits(built, cpw):
    """an all-zero channel; a noise-only channel (a crossing and a slip in almost every symbol) that hunts through the 1800 symbols
    of the no-carrier count, where the pass yields and comes back; samples beyond 1.25 x max in the gaps (the `!(x > hl)` side of the
    crossing test); inverted polarity; a carrier that appears after 2000 symbols of silence, so that the filter's cold start keeps
    the pass away; ordinary traffic beside them"""
    B, n = 8, 30000
    rng = np.random.default_rng(11)
    x = np.zeros((B, n), np.float32)
    x[1] = rng.normal(0, 6000, n)
    dib, sc = _short_frames(4, n, (10, 40))
    x[2] = _mod(dib, sc, 215, 90.0, 12, n)
    at = rng.integers(0, n, 400)
    x[2, at] += rng.choice([-1.0, 1.0], 400) * rng.uniform(9000, 30000, 400)   # (levels +-3 x 7000 / 3: far beyond 1.25 x max)
    x[3] = -_mod(dib, sc, 318, 1200.0, 13, n)
    s = _mod(dib, sc, 150, 90.0, 14, n)
    x[4, 20000:] = s[:n - 20000]
    x[5, 20003:] = rng.normal(0, 300, n - 20003) + s[:n - 20003]
    x[5, :20003] = rng.normal(0, 300, 20003)                                   # (noise instead of silence in front of the carrier)
    for c in (6, 7):
        t = _traffic(500 + c, n, [90.0, 4000.0][c % 2])
        x[c, :len(t)] = t
    out = _three_ways(x, cpw, (0, 1, 2, 3, 4, 5))
    assert int(out[2][0]) > 0 and (out[1][0] & 2).sum() == 0 and (out[1][1] & 2).sum() == 0
    for c in (2, 3, 4, 5):
        assert (out[1][c] & 2).sum() >= 3, c


@pytest.mark.gpu
@pytest.mark.parametrize("cpw", [4, 8])
def test_tile_and_call_edges(built, cpw):
    """the same stream as one call and as consecutive calls of 1, 127, 128, 129 and 300 samples on one object: symbol starts lie
    in the previous tile, symbols do not fit the tile (the lane waits for the next one), a pass ends at the record capacity of a
    short call - and the calls' outputs joined are the one call's"""
    B, n = 8, 7000
    x = np.zeros((B, n), np.float32)
    for c in range(B):
        dib, sc = _short_frames(20 + c // 2, n, (4, 25))
        x[c] = _mod(dib, sc, 90 + 11 * c, [90.0, 2500.0][c % 2], 30 + c, n)
    x[6] = np.random.default_rng(6).normal(0, 5000, n)
    whole = _three_ways(x, cpw, (0, 1, 6))
    _same(whole, _three_ways(x, cpw, (), calls=(1, 127, 128, 129, 300)), "one call against consecutive short calls")


def test_first_extrema_step_needs_no_second_values():
    """The pass's extrema reduction keeps the two smallest and the two largest symbols by insertion (two_min_insert /
    two_max_insert, ddn_slicer_dev.h).  In its first step every lane's second values are still +inf / -inf; the step leaves their
    insertion out.  Restated here in float32: inserting +inf into a pair of minima (-inf into maxima) changes neither value's
    bits, whatever the pair holds - ties, +0 / -0, infinities, NaN, and fewer than two live values (the pair still at its start)."""
    def ins_min(v, a1, a2):
        c1, c2 = v < a1, v < a2
        return (v if c1 else a1), (a1 if c1 else (v if c2 else a2))

    def ins_max(v, b1, b2):
        c1, c2 = v > b1, v > b2
        return (v if c1 else b1), (b1 if c1 else (v if c2 else b2))

    f = np.float32
    rng = np.random.default_rng(0)
    special = [f(0.0), f(-0.0), f(np.inf), f(-np.inf), f(np.nan), f(1.0), f(-1.0), f(3.4e38), f(1e-45)]
    vals = special + [f(v) for v in rng.normal(0, 7000, 40)]
    bits = lambda v: np.float32(v).view(np.uint32)
    with np.errstate(invalid="ignore"):
        for own in vals:
            for other in vals:
                a = ins_min(other, own, f(np.inf))           # the first step proper: the neighbour's first value
                b = ins_max(other, own, f(-np.inf))
                a2 = ins_min(f(np.inf), *a)                  # ... and what it leaves out: the neighbour's second value
                b2 = ins_max(f(-np.inf), *b)
                assert [bits(v) for v in a] == [bits(v) for v in a2], (own, other)
                assert [bits(v) for v in b] == [bits(v) for v in b2], (own, other)
