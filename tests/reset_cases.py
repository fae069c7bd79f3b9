"""Inputs of the receive loops' reset tests (tests/test_reset_gpu.py) and of the CPU test that holds their premise on the oracle
(tests/test_reset_cases.py): two unrelated streams per case - X, what the object sees before the reset, and Y, what it and a fresh
object see afterwards.  X is scaled by 0.4, negated, and cut so that it ends inside a frame with a sync held.  TEST INFRASTRUCTURE -
never imported by the product."""
import numpy as np

import ddn
import orc
import rx4

# ---- ddn_p25_rx ----------------------------------------------------------------------------------------------------------------------
P25_B, P25_N, P25_FRAME = 70, 6000, 432


def p25_case():
    """-> x [B][n], y [B][2 n], per-channel lock lengths (none shorter than 200 symbols: the second frame of X, accepted round
    sample 4800, is still being read at sample 6000)"""
    x = orc.synth_p25_disc(51, P25_B, P25_N, frame_dibits=P25_FRAME, negative=True)[0] * np.float32(0.4)
    y = orc.synth_p25_disc(53, P25_B, 2 * P25_N, frame_dibits=P25_FRAME)[0]
    locks = np.array([[P25_FRAME - 24, 200, 250, 300][c % 4] for c in range(P25_B)], np.int32)
    return x, y, locks


def p25_handler_x():
    """X of the handlers-on cases -> [B][n]: synth_p25_disc's frames carry random NIDs, on which a handler gives its frame up at
    once; these are well-formed three-block TSDUs back to back (tests/p25gen.py), negated and scaled like the other X, and a TSDU
    is 3600 samples long, so sample 6000 falls inside the second one of every channel: the handler holds a decoded NID and is in the
    middle of its blocks, its words and its history ring away from their reset values"""
    import p25gen
    x = np.zeros((P25_B, P25_N), np.float32)
    for c in range(P25_B):
        rng = np.random.default_rng(900 + c)
        dib = p25gen.make_frames(rng, 3, 0x293, crc=True, blocks=3)[0]
        s = p25gen.modulate_disc(dib, lead=150 + 13 * (c % 17), noise=150.0, seed=c)[:P25_N]
        x[c, :len(s)] = s
    return x * np.float32(-0.4)


def p25_oracle(handlers, lock):
    return orc.OracleP25Rx(lock_symbols=-1 if handlers else int(lock), use_filter=1)


# ---- ddn_fsk4_rx ---------------------------------------------------------------------------------------------------------------------
FSK4_B, FSK4_N = 5, 12000
FSK4_NAMES = ("dmr", "nxdn48", "m17", "dstar")
# where X is cut from its capture: the slice ends 1000 samples after this sample (one at which the oracle holds a sync)
_X_AT = {"dmr": 30000, "nxdn48": 54000}


def fsk4_case(name):
    """-> dict(proto, rf_mod, handlers, lock [4], oracle = a factory, x [5][FSK4_N], y [5][2 * FSK4_N]).  Y is the capture slice
    tests/test_nonfinite_gpu.py uses; X comes from elsewhere - for DMR from a capture with another colour code (2, Y's is 0), so
    that the handlers' colour-code words are away from their reset value of 16"""
    import fuzz_rx4 as fz
    if name in fz.ROWS:
        row, s = fz.ROWS[name], fz.scan(name)
        disc = x_src = s["disc"]
        at, x_at = int(s["sync_at"][0]), int(s["sync_at"][len(s["sync_at"]) // 2])
        proto, rf_mod, handlers = row.gpu_proto, row.rf_mod0, False
        lock = row.default_lock()
        lock[0] -= 2                                     # not the default: a reset that restored the configuration's would show
        oracle = lambda: row.oracle(rf_mod, 48000, lock)
    elif name == "dmr":
        disc, x_src = rx4.capture_disc("iq_dmr_t3_ras_cc.npz", 2), rx4.capture_disc("iq_dmr_voice.npz", 2)
        at, x_at, proto, rf_mod, handlers = 61000, _X_AT[name], ddn.FSK4_DMR, 2, True
        lock = [120, 54 + 288 * 6, 12, 0]
        oracle = lambda: rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, rf_mod=rf_mod, lock=lock, handler=1))
    else:
        disc = x_src = rx4.capture_disc("iq_nxdn48.npz", 1)
        at, x_at, proto, rf_mod, handlers = 61000, _X_AT[name], ddn.FSK4_NXDN48, 0, False
        lock = [180, 0, 0, 0]
        oracle = lambda: rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_NXDN48, lock=lock))
    B, n = FSK4_B, FSK4_N
    at = max(0, min(at - 1500, len(disc) - 2 * n - 200))
    y = np.stack([disc[at + 37 * c:at + 37 * c + 2 * n] for c in range(B)]).astype(np.float32)
    xs = max(0, min(x_at - n + 1000, len(x_src) - n - 200))
    # (DMR keeps its polarity: the handlers then settle on the capture's colour code)
    x = np.stack([x_src[xs + 37 * c:xs + 37 * c + n] for c in range(B)]).astype(np.float32) * np.float32(0.4 if name == "dmr" else -0.4)
    return dict(proto=proto, rf_mod=rf_mod, handlers=handlers, lock=lock, oracle=oracle, x=x, y=y)


def events4(rows):
    """oracle event rows -> int64 [n][4] {pos, kind, a, b | c << 16} as the device packs them"""
    return np.array([[e[0], e[1], e[2], (e[3] & 0xFFFF) | ((e[4] & 0xFFFF) << 16)] for e in rows], np.int64).reshape(-1, 4)


EVENT_MASK = np.array([-1, -1, -1, 0xFFFFFFFF])
