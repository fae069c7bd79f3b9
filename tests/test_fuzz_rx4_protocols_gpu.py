"""Differential fuzz of the fsk4 receive loop's six newer protocols - NXDN96, M17, YSF, dPMR, D-STAR, EDACS - against their CPU
loops, bit for bit: traffic from tests/fuzz_rx4.py (tests/test_fuzz_rx4_traffic.py holds it to its floors without a GPU), every
wavefront shape, batches that leave the last wavefront partly filled, 48 ksps and both ends of the accepted samples-per-symbol range,
per-channel lock lengths, carrier loss, and call cuts at a single sample, inside a symbol, on a staging-tile edge and right behind a
sync.  DDN_FUZZ_BASE=k shifts the seeds."""
import numpy as np
import pytest

import ddn
import fuzz_rx4 as fz
from test_rx4_gpu import check_channel

pytestmark = pytest.mark.gpu
POISON = 0xA5


class DeviceLoop:
    """ddn_fsk4_rx_run on device buffers of exactly ddn_fsk4_rx_max_symbols / _max_syncs per channel, the per-sync thresholds beside
    them, and one poisoned row behind the last channel's that has to come back as it went"""

    def __init__(self, row, B, rf_mod, out_rate, lock, cpw, use_filter=1, inverted=0):
        self.l, self.B = ddn.lib(), B
        self.rx = ddn.Fsk4Rx(B, row.gpu_proto, rf_mod=rf_mod, inverted=inverted, use_matched_filter=use_filter, out_rate=out_rate)
        lock = np.ascontiguousarray(lock, np.int32)
        assert lock.shape == (B, 4) and self.l.ddn_fsk4_rx_set_lock_symbols(self.rx.h, lock.ctypes.data) == 0
        assert self.l.ddn_fsk4_rx_set_channels_per_wave(self.rx.h, cpw) == 0
        self.sps, self.win = out_rate // row.sym_rate, row.win_len

    def run(self, x):
        import torch
        l, B = self.l, self.B
        n = x.shape[1]
        ms, my = l.ddn_fsk4_rx_max_symbols(self.rx.h, n), l.ddn_fsk4_rx_max_syncs(self.rx.h, n)
        assert (ms, my) == (fz.max_symbols(n, self.sps), fz.max_syncs(n, self.sps, self.win))
        d = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()           # exactly B * n samples: nothing behind the last one
        u8 = lambda *shape: torch.full((B + 1,) + shape, POISON, dtype=torch.uint8, device="cuda")
        i32 = lambda *shape: torch.full((B + 1,) + shape, -0x5A5A5A5B, dtype=torch.int32, device="cuda")
        rec, fl, pay, spat, pre, prel = u8(ms, 10), u8(ms), u8(ms, 2), u8(my), u8(my, ddn.FSK4_PRE), u8(my, ddn.FSK4_PRE)
        cnt, ns, spos = i32(), i32(), i32(my)
        thr = torch.full((B + 1, my, 5), float("nan"), dtype=torch.float32, device="cuda")
        p = lambda t: t.data_ptr()
        assert l.ddn_fsk4_rx_set_sync_thresholds(self.rx.h, p(thr)) == 0
        rc = l.ddn_fsk4_rx_run(self.rx.h, p(d), n, p(rec), p(fl), p(pay), p(cnt), ms, p(spos), p(spat), p(pre), p(prel), p(ns), my, None)
        torch.cuda.synchronize()
        assert rc == 0
        assert l.ddn_fsk4_rx_set_sync_thresholds(self.rx.h, None) == 0
        h = lambda t: t.cpu().numpy()
        got = dict(rec=h(rec), fl=h(fl), pay=h(pay), cnt=h(cnt), sync_pos=h(spos), sync_pat=h(spat), pre=h(pre), pre_rel=h(prel),
                   n_sync=h(ns), thr=h(thr), ms=ms, my=my)
        for k in ("rec", "fl", "pay", "sync_pat", "pre", "pre_rel"):
            assert (got[k][B] == POISON).all(), k                       # the row behind the last channel's
        for k in ("cnt", "n_sync", "sync_pos"):
            assert (got[k][B] == -0x5A5A5A5B).all(), k
        assert np.isnan(got["thr"][B]).all()
        assert (got["cnt"][:B] >= 0).all() and (got["cnt"][:B] <= ms).all()
        assert (got["n_sync"][:B] >= 0).all() and (got["n_sync"][:B] <= my).all()
        return got

    def check(self, got, ch, cpu, want, where):
        """records, flags, payload, reliabilities, hand-overs; the thresholds each sync left; the thresholds the call left"""
        try:
            check_channel(got, ch, want)
        except AssertionError as e:
            raise AssertionError("%r: %s" % (where, e)) from e
        ns = len(want["sync_pos"])
        assert np.array_equal(got["thr"][ch, :ns].view(np.uint32), want["sync_thr"].view(np.uint32)), where
        assert np.array_equal(self.rx.thresholds(ch).view(np.uint32), cpu.thresholds().view(np.uint32)), where


def run_case(c):
    """one built case through the device loop and the oracles, call by call -> syncs seen"""
    gpu = DeviceLoop(c.row, c.B, c.rf_mod, c.out_rate, c.lock, c.cpw, c.use_filter, c.inverted)
    cpu = fz.oracles(c)
    n_sync = 0
    for a, b in fz.calls(c):
        got = gpu.run(c.x[:, a:b])
        for ch in range(c.B):
            want = cpu[ch].run(c.x[ch, a:b], max_sync=got["my"])
            gpu.check(got, ch, cpu[ch], want, (c.name, c.case, ch, a, b))
            n_sync += len(want["sync_pos"])
    gpu.rx.close()
    return n_sync


@pytest.mark.parametrize("case", range(fz.N_CASES))
@pytest.mark.parametrize("name", fz.PROTOCOLS)
def test_fuzz_rx4_protocols(built, name, case):
    assert run_case(fz.build(name, case)) >= 3


@pytest.mark.parametrize("name", fz.PROTOCOLS)
def test_fuzz_rx4_densest_syncs(built, name):
    """The sync table cannot fill: the hunt restarts with an empty window, so two accepted syncs lie at least one sync word apart, and
    a call of K symbols holds at most (K - 1) / win_len + 1 of them - below ddn_fsk4_rx_max_syncs = max_symbols / win_len + 2 for every
    protocol, as the oracle shows on the densest streams there are (tests/test_fuzz_rx4_traffic.py: a long M17 preamble under lock
    lengths {1, 1, 0, 0}, EDACS frames back to back under lock 1, every protocol's sync words one lock symbol apart).  No protocol has
    a saturation case for that reason; what is compared here is those densest streams, where the table is as full as it gets."""
    c = fz.build_densest(name)
    n_sync = run_case(c)
    assert n_sync >= 20 * c.B
