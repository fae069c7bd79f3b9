"""dPMR (-fm) on the device: DDN_FSK4_DPMR as the fsk4 loop's sixth protocol (12-symbol FS2 word in the polarity -xd selects,
dpmr_filter, 372 dibits behind a sync) against the profile-driven oracle loop, on the reference's capture and across call splits."""
import numpy as np
import pytest

import ddn
import dpmr
import rx4
from test_rx4_gpu import check_channel, rec4_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cpw", [0, 1, 4])
@pytest.mark.parametrize("inverted,rf_mod", [(0, 2), (1, 2), (0, 0)])
def test_dpmr_loop_bit_exact_with_call_splits(built, cpw, inverted, rf_mod):
    disc = rx4.capture_disc("iq_dpmr.npz", 1)
    n = len(disc)
    B = 5
    rng = np.random.default_rng(7)
    x = np.zeros((B, n), np.float32)
    for c in range(B):
        d = 53 * c
        x[c, :d] = rng.standard_normal(d) * 500
        x[c, d:] = disc[:n - d]
    x[1] = -x[1]            # the other polarity: the other word locks
    x[4, :30000] = 0
    for use_filter in (1, 0):
        gpu = ddn.Fsk4Rx(B, ddn.FSK4_DPMR, rf_mod=rf_mod, inverted=inverted, use_matched_filter=use_filter)
        if cpw:
            assert ddn.lib().ddn_fsk4_rx_set_channels_per_wave(gpu.h, cpw) == 0
        cpu = [rx4.OracleFsk4Rx(dpmr.profile(inverted, use_filter=use_filter, rf_mod=rf_mod)) for _ in range(B)]
        cuts = [0, 4097, 4097 + 63, 60000, 60001, 150000, 150000 + 7 * 384 * 20 + 13, n]
        n_sync = np.zeros(B, np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            got = gpu.run_host(x[:, a:b])
            for c in range(B):
                want = cpu[c].run(x[c, a:b], max_sync=got["sync_pos"].shape[1])
                check_channel(got, c, want)
                n_sync[c] += len(want["sync_pos"])
                assert np.array_equal(gpu.thresholds(c).view(np.uint32), cpu[c].thresholds().view(np.uint32)), (c, a)
        locked = 1 if inverted == 0 else 0          # the channel whose polarity matches the hunted word
        assert n_sync[locked] >= 50, n_sync
        assert n_sync[1 - locked] < 10, n_sync


def test_dpmr_capture_src_1601621_from_device_records(built):
    """DECODE_IQ_DPMR (tests/CMakeLists.txt:8950): plain -fm (the FS2 word as written, GFSK rules) on the device; the records
    behind its syncs, through the restatement's identity rules, print "Src=1601621" and equal the oracle loop's"""
    disc = rx4.capture_disc("iq_dpmr.npz", 1)
    gpu = ddn.Fsk4Rx(1, ddn.FSK4_DPMR, rf_mod=2)
    got = gpu.run_host(disc[None, :])
    k = int(got["cnt"][0])
    r4, _ = rec4_of(got["rec"][0, :k])
    sp = got["sync_pos"][0, :int(got["n_sync"][0])]
    want = rx4.OracleFsk4Rx(dpmr.profile(0)).run(disc)
    assert np.array_equal(sp, want["sync_pos"]) and np.array_equal(r4[:, 0], want["rec4"][:, 0])
    srcs = [sf["src"] for _, sf in dpmr.decode_stream(r4[:, 0], sp)]
    assert "1601621" in srcs and all(s == "1601621" for s in srcs[srcs.index("1601621"):])


def test_dpmr_rejects_handlers_and_accepts_inverted(built):
    l = ddn.lib()
    for inverted in (0, 1):
        b = ddn.Fsk4Rx(2, ddn.FSK4_DPMR, inverted=inverted)
        assert l.ddn_fsk4_rx_set_handlers(b.h, 1) == -1      # DDN_EINVAL: a fixed count, no handler family
        b.close()
    with pytest.raises(ddn.DdnError, match=r"rc=-1 ddn_fsk4_rx_create: bad configuration"):
        ddn.Fsk4Rx(2, ddn.FSK4_NXDN48, inverted=1)        # DDN_EINVAL: inverted is DMR's and dPMR's only
