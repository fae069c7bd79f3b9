"""The CPU side of the P25 chain object's CQPSK tests (tests/test_chain_cqpsk_gpu.py; floors in
tests/test_chain_cqpsk_short_calls_traffic.py): the whole-stream oracle with the demodulator's blocks cut the way the chain cuts them, and
the short-call cases.  No device, no bindings."""
import numpy as np

import orc


def oracle_stream(iq, n_total, n_call):
    x = ((iq[:n_total].astype(np.float32) - 127.5) * np.float32(1.0 / 127.5)).astype(np.float32)
    fe = orc.OracleCqpskFe(rate=48000)          # a call = consecutive full_demod() blocks of 8192 + a shorter last one, like the chain's
    sym = np.concatenate([fe.run(x[k:k + n_call], 8192) for k in range(0, n_total, n_call)])
    rx = orc.OracleCqRx(orc.CQ_P25P1)
    rec, fl = rx.run(sym)
    return sym, rec, fl, rx.events.rows(), rx.events.data()


# calls at or below the carry (960 symbols = 9600 samples): a third of it with the boundaries off the symbol edges, one demodulator block,
# one block plus the shortest ragged block the demodulator takes, exactly the carry; the voice capture at the shortest, so that an LDU
# (864 symbols) crosses three calls or more.  The captures are 96000 samples (2 s) each and are run whole - there is nothing to cut a
# slice from: 29 calls at 3201 samples, each case under 0.2 s on the device.  tests/test_chain_cqpsk_short_calls_traffic.py holds the
# traffic floors on the CPU.
CARRY = 960
SHORT_CALLS = [("iq_p25p1_cqpsk_cc.npz", 3201), ("iq_p25p1_cqpsk_cc.npz", 8192), ("iq_p25p1_cqpsk_cc.npz", 8196),
               ("iq_p25p1_cqpsk_cc.npz", 9600), ("iq_p25p1_cqpsk_vc.npz", 3201)]


def symbols_per_call(iq, n_total, n_call):
    """how many new records every call brings, by the oracle's demodulator"""
    x = ((iq[:n_total].astype(np.float32) - 127.5) * np.float32(1.0 / 127.5)).astype(np.float32)
    fe = orc.OracleCqpskFe(rate=48000)
    return np.array([len(fe.run(x[k:k + n_call], 8192)) for k in range(0, n_total, n_call)])
