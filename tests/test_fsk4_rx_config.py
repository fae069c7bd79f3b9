"""The fsk4 receive loop's host object against its protocol table (csrc/ddn_fsk4_proto.h): what ddn_fsk4_rx_create accepts and refuses,
which protocols have a handler family, and the two sizes the host derives from a protocol's symbol rate and sync window."""
import ctypes as C
import itertools

import pytest

import ddn

EINVAL, ENODEV, ERANGE = -1, -2, -5
RATES = (0, 19200, 33600, 38400, 43200, 48000, 52800, 96000, 100800, 105600)  # both sides of 8..21 at 2400 / 4800 and of 5..10 at 9600


def _create(protocol, rf_mod=0, inverted=0, out_rate_hz=48000, n_channels=2):
    h = C.c_void_p()
    cfg = ddn.Fsk4RxConfig(n_channels, out_rate_hz, protocol, rf_mod, inverted, 1, (C.c_int * 4)())
    return ddn.lib().ddn_fsk4_rx_create(C.byref(cfg), C.byref(h)), h


def _expected(protocol, rf_mod, inverted, rate, n_channels, have_device):
    if n_channels <= 0 or rate <= 0 or not 1 <= protocol <= 8 or rf_mod not in (0, 2):
        return EINVAL
    if inverted and protocol not in (ddn.FSK4_DMR, ddn.FSK4_DPMR):
        return EINVAL
    if protocol == ddn.FSK4_EDACS:
        if rate % 9600 != 0 or not 5 <= rate // 9600 <= 10:
            return ERANGE
    else:
        sym_rate = 2400 if protocol in (ddn.FSK4_NXDN48, ddn.FSK4_DPMR) else 4800
        if not 8 <= rate // sym_rate <= 21:
            return ERANGE
    return 0 if have_device else ENODEV


def test_fsk4_rx_configuration_is_checked_before_any_device_is_touched(built):
    """ddn_fsk4_rx_create over protocol x rf_mod x inverted x out_rate_hz x n_channels: DDN_EINVAL for a configuration no protocol
    takes, then DDN_ERANGE for a samples-per-symbol count outside the protocol's range - on a box without a GPU too; a good one
    without a device is DDN_ENODEV (never a CPU path)"""
    import torch
    have = torch.cuda.is_available()
    l = ddn.lib()
    bad = []
    for proto, rf_mod, inv, rate, nch in itertools.product(range(10), (0, 1, 2), (0, 1), RATES, (0, 2)):
        rc, h = _create(proto, rf_mod, inv, rate, nch)
        if rc == 0:
            l.ddn_fsk4_rx_destroy(h)
        if rc != _expected(proto, rf_mod, inv, rate, nch, have):
            bad.append((proto, rf_mod, inv, rate, nch, rc))
        elif rc == EINVAL:
            assert b"ddn_fsk4_rx_create: bad configuration" in l.ddn_last_error()
    assert not bad, bad


WHOLE = {1: 10, 2: 20, 3: 10, 4: 10, 5: 10, 6: 20, 7: 10, 8: 5}       # samples per symbol at 48 ksps
WIN_LEN = {1: 24, 2: 10, 3: 10, 4: 8, 5: 20, 6: 12, 7: 24, 8: 48}     # symbols of the sync window


@pytest.mark.gpu
@pytest.mark.parametrize("protocol", range(1, 9))
def test_fsk4_rx_handler_families_and_sizes(built, protocol):
    """ddn_fsk4_rx_set_handlers: DMR, NXDN48 and NXDN96 have a handler family, the fixed-count protocols are refused where the object
    is configured (not at the first run); ddn_fsk4_rx_max_syncs follows the protocol's symbol rate and sync window"""
    l = ddn.lib()
    rc, h = _create(protocol)
    assert rc == 0
    try:
        if protocol in (ddn.FSK4_DMR, ddn.FSK4_NXDN48, ddn.FSK4_NXDN96):
            assert l.ddn_fsk4_rx_set_handlers(h, 1) == 0
        else:
            assert l.ddn_fsk4_rx_set_handlers(h, 1) == EINVAL
            assert b"no handler family" in l.ddn_last_error()
        assert l.ddn_fsk4_rx_max_syncs(h, 4800) == (4800 // (WHOLE[protocol] - 1) + 2) // WIN_LEN[protocol] + 2
    finally:
        l.ddn_fsk4_rx_destroy(h)
    if protocol == ddn.FSK4_DMR:
        rc, h = _create(protocol, inverted=1)
        assert rc == 0
        try:
            assert l.ddn_fsk4_rx_set_handlers(h, 1) == EINVAL
        finally:
            l.ddn_fsk4_rx_destroy(h)
