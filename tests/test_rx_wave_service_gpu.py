"""Handler mode of the receive loop: the order in which the helper waves serve the two recurrence waves of a workgroup changes no
output.  A channel has one request open at most and its own event list, so records, flags, counts, events and event data equal the
oracle's bit for bit whichever pending request the handler wave takes first and whichever due half the staging wave stages first -
with all lanes posting in one trip, with posts one symbol apart, with partly filled waves, with voice and control channels side by
side, in one call and across a call boundary inside a frame.  Every case also runs under the other orders of ddn_rx.hip
(ddn_p25_rx_set_debug_flags bits 2 / 4 / 8 / 16 / 32) and must give identical arrays; those orders are compiled into builds with
-DDDN_RXW_ORDERS=1 (the instrumented variant of tools/build_variant.sh has them: DDN_LIB_PATH=... runs this file against it), the
product build keeps lowest-first and reads the bits as nothing."""
import numpy as np
import pytest

import ddn
import orc
import p25gen

pytestmark = pytest.mark.gpu

N = 12000            # discriminator samples per channel: four to six TSDUs
# ddn_p25_rx_set_debug_flags: the recurrence wave that is behind first (handler wave, staging wave); oldest request first; both
# waves highest first
ORDERS = (16 | 32, 8, 2 | 4)
_WANT = {}


def _control(seed=5):
    """one- to three-block TSDUs back to back"""
    rng = np.random.default_rng(seed)
    return np.concatenate([p25gen.make_frames(rng, 1, 0x293, crc=True, blocks=b)[0] for b in (3, 1, 2, 3, 2, 1, 3)])


def _voice(seed=6):
    import mbe
    rng = np.random.default_rng(seed)
    frames = np.stack([mbe.imbe_encode(b) for b in mbe.random_imbe_bits(rng, (18,))])
    return p25gen.make_ldus(rng, 2, 0x293, frames)[0]


def _rows(dibits, leads, noise=100.0, seed=11):
    """the same dibit stream and the same noise on every channel, `leads[c]` samples of lead each"""
    x = np.zeros((len(leads), N), np.float32)
    for c, lead in enumerate(leads):
        s = p25gen.modulate_disc(dibits, lead=int(lead), noise=noise, seed=seed)[:N]
        x[c, :len(s)] = s
    return x


def _oracle(row):
    key = row.tobytes()
    if key not in _WANT:      # computed once per distinct channel, shared by the cases, never written to
        rx = orc.OracleP25Rx(lock_symbols=-1, use_filter=1)
        sym, rec, fl = rx.run(row)
        ev = [[e[0], e[1], e[2], (e[3] & 0xFFFF) | ((e[4] & 0xFFFF) << 16)] for e in rx.events.rows()]
        _WANT[key] = (sym, rec, fl, np.array(ev, np.int64).reshape(-1, 4), rx.events.data())
    return _WANT[key]


def _run(x, cpw, dbg, splits):
    """-> per channel (records10, flags, events with output indices counted from the first call, event data) over all the calls"""
    B = x.shape[0]
    rx = ddn.P25Rx(B, use_matched_filter=1, channels_per_wave=cpw, handlers=True, max_events=256, debug_flags=dbg)
    parts = [[[], [], [], []] for _ in range(B)]
    base = np.zeros(B, np.int64)
    for a, b in zip(splits[:-1], splits[1:]):
        rec, fl, cnt = rx.run(np.ascontiguousarray(x[:, a:b]))
        for c in range(B):
            e = rx.events[c, :rx.n_events[c]].astype(np.int64)
            e[:, 0] += base[c]
            for lst, v in zip(parts[c], (rec[c, :cnt[c]], fl[c, :cnt[c]], e, rx.event_data[c, :rx.n_events[c]])):
                lst.append(np.array(v))
            base[c] += cnt[c]
    return [tuple(np.concatenate(p) for p in parts[c]) for c in range(B)]


def _case(x, cpw, splits=(0, N), min_events=4):
    got = _run(x, cpw, 0, splits)
    for dbg in ORDERS:                       # order independence: identical arrays
        other = _run(x, cpw, dbg, splits)
        for c in range(x.shape[0]):
            for a, b in zip(got[c], other[c]):
                assert a.shape == b.shape and np.array_equal(a, b), (dbg, c)
    for c in range(x.shape[0]):
        rec, fl, ev, evd = got[c]
        sym_o, rec_o, fl_o, ev_o, evd_o = _oracle(x[c])
        assert len(fl) == len(sym_o), (c, len(fl), len(sym_o))                       # counts
        r4, sy = orc.unpack_records10(rec)
        assert np.array_equal(fl, fl_o), (c, np.flatnonzero(fl != fl_o)[:5])          # flags
        assert np.array_equal(sy.view(np.uint32), sym_o.view(np.uint32)), c          # records
        assert np.array_equal(r4, rec_o), c
        mask = np.array([-1, -1, -1, 0xFFFFFFFF])
        assert len(ev) == len(ev_o) and np.array_equal(ev & mask, ev_o & mask), (c, ev[:6], ev_o[:6])   # events
        assert np.array_equal(evd, evd_o), (c, np.flatnonzero((evd != evd_o).any(axis=1))[:4])          # event data
        assert len(ev) >= min_events, (c, len(ev))      # the case did exercise the handler wave


@pytest.mark.parametrize("B,cpw", [(8, 8), (16, 16)])
def test_all_lanes_post_in_the_same_trip(built, B, cpw):
    _case(_rows(_control(), [230] * B), cpw)


def test_posts_one_symbol_apart(built):
    _case(_rows(_control(), [230 + 10 * c for c in range(8)]), 8)


@pytest.mark.parametrize("B", [5, 12])
def test_partly_filled_waves(built, B):
    """B = 5: the second recurrence wave has one lane; B = 12: the second workgroup has no channel on its second wave"""
    _case(_rows(_control(), [230 + 10 * (c % 3) for c in range(B)]), 8)


@pytest.mark.parametrize("splits", [(0, N), (0, 6005, N)])
def test_voice_and_control_side_by_side(built, splits):
    """voice LDUs on the even channels, TSDUs on the odd ones; the second form splits the run inside a frame"""
    xv = _rows(_voice(), [230, 260, 290, 320])
    xc = _rows(_control(), [230, 240, 250, 260])
    x = np.empty((8, N), np.float32)
    x[0::2] = xv
    x[1::2] = xc
    _case(x, 8, splits, min_events=2)
