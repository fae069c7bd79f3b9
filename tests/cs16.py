"""Helpers of the cs16 (16-bit integer I/Q) tests: the widening every comparison goes through, deterministic int16 streams salted
with the extreme pairs, and the conversion of a cu8 capture to cs16.  TEST INFRASTRUCTURE, no tests here.

The device widens a cs16 pair as float(s) * 2^-15 (soapy_copy_cs16_samples, src/io/radio/rtl_device.cpp:1247-1264).  Every int16 is
exact in binary32 and the scale is a power of two, so widen() below gives the very floats the kernels must produce, and every
comparison built on it is bit for bit."""
import ctypes as C

import numpy as np

import orc

# the pairs a wrong sign extension, a wrong half or a wrong shift cannot survive: extremes of both signs in both halves, +-1 (all
# ones against a single one in a half), zero
SALT = np.array([(-32768, 32767), (32767, -32768), (-1, 1), (1, -1), (0, 0), (-32768, -32768)], np.int16)
TILE = 256   # time tile of the fused front-end kernel: its first tile is loaded synchronously, the later ones prefetched
CARRY = 72   # DDN_CARRY_LEN: the samples of a call the next one looks back on


def widen(x):
    """int16 [...] -> float32 [...], exactly"""
    x = np.asarray(x)
    assert x.dtype == np.int16
    return x.astype(np.float32) * np.float32(2.0 ** -15)


def cu8_to_cs16(u8):
    """256 * (u - 127.5): the cu8 stream at a gain of 127.5 / 128 with no offset; fits int16 for every u"""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8
    v = (u8.astype(np.int32) - 128) * 256 + 128
    assert v.min() >= -32768 and v.max() <= 32767
    return v.astype(np.int16)


def salt_positions(n, block_len, calls=None):
    """where the SALT run (len(SALT) consecutive samples) goes: inside the first tile, inside a prefetched tile, inside the last CARRY
    samples of every call (`calls` = the calls' lengths, default one call of n) and across a block edge"""
    k = len(SALT)
    pos = [7, TILE + 41, block_len - k // 2]
    end = 0
    for c in (calls or [n]):
        end += c
        pos.append(end - CARRY // 2)
    return sorted({p for p in pos if 0 <= p and p + k <= n})


def salt(x, positions):
    """x int16 [B, n, 2], in place; channel c's run starts c samples later (so channels differ and one of them meets every edge)"""
    B, n = x.shape[0], x.shape[1]
    for c in range(B):
        for p in positions:
            q = min(p + (c % 3), n - len(SALT))
            x[c, q:q + len(SALT)] = SALT
    return x


def synth_c4fm_cs16(ch_first, n_ch, n, block_len, calls=None, sps=10):
    """orc.synth_c4fm_cu8 scaled to int16 and salted -> int16 [n_ch, n, 2]"""
    x = cu8_to_cs16(orc.synth_c4fm_cu8(ch_first, n_ch, n, sps=sps))
    return salt(x, salt_positions(n, block_len, calls))


def synth_dqpsk_cs16(seed, n_ch, n_sym, sps, block_len, calls=None):
    """orc.synth_dqpsk_f32 (amplitude 0.6) scaled to int16 at 30000 per unit and salted -> int16 [n_ch, n, 2]"""
    f = orc.synth_dqpsk_f32(seed, n_ch, n_sym, sps)
    x = np.clip(np.rint(f.astype(np.float64) * 30000.0), -32768, 32767).astype(np.int16)
    return salt(x, salt_positions(x.shape[1], block_len, calls))


class _FskState(C.Structure):  # orc_fsk_state (oracle/ddn_oracle.h)
    _fields_ = [("prev_i", C.c_float), ("prev_q", C.c_float), ("have_prev", C.c_int), ("dc_est", C.c_float), ("peak_est", C.c_float)]


_ORC_MAX_TAPS = 144
# offset of orc_front_end.fsk: five ints and a float, taps / hist_i / hist_q, hb_hist_i / hb_hist_q [10][30]
_FSK_OFFSET = 6 * 4 + 3 * _ORC_MAX_TAPS * 4 + 2 * 10 * 30 * 4


def oracle_fsk_state(fe):
    """the carried modem state of an orc.OracleFrontEnd as ddn_batch_get_fsk_state reports it: float32 {prev_i, prev_q, have_prev, dc,
    peak}"""
    s = _FskState.from_buffer(fe.buf, _FSK_OFFSET)
    return np.array([s.prev_i, s.prev_q, float(s.have_prev), s.dc_est, s.peak_est], np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class F32FrontEnd:
    """an orc.OracleFrontEnd behind the `run_cu8` name chain_oracle.run_channel / chain_stream.run_stream call, taking floats: lets
    the whole-stream CPU restatement run on widened cs16"""

    def __init__(self, **kw):
        self.fe = orc.OracleFrontEnd(**kw)

    def run_cu8(self, iq_f32, block_len):
        assert np.asarray(iq_f32).dtype == np.float32
        return self.fe.run_f32(iq_f32, block_len)


def write_capture(path, samples, sample_format, rate=48000):
    """a dsd-neo-iq capture (data file + JSON sidecar, metadata version 1) holding `samples` ([n, 2] uint8 / int16 / float32)"""
    import json
    import os
    samples = np.ascontiguousarray(samples)
    assert {"cu8": np.uint8, "cs16": np.int16, "cf32": np.float32}[sample_format] == samples.dtype
    samples.astype(samples.dtype.newbyteorder("<")).tofile(path)
    meta = {"format": "dsd-neo-iq", "version": 1, "sample_format": sample_format, "iq_order": "IQ",
            "endianness": "none" if sample_format == "cu8" else "little",
            "capture_stage": "post_mute_pre_widen", "sample_rate_hz": rate, "center_frequency_hz": 851000000,
            "capture_center_frequency_hz": 851000000, "ppm": 0, "tuner_gain_tenth_db": 0, "rtl_dsp_bw_khz": 0,
            "base_decimation": 1, "post_downsample": 1, "demod_rate_hz": rate, "offset_tuning_enabled": False,
            "fs4_shift_enabled": False, "combine_rotate_enabled": False, "muted_bytes_excluded": True,
            "contains_retunes": False, "capture_retune_count": 0, "source_backend": "soapy", "source_args": "driver=test",
            "capture_started_utc": "2026-07-30T00:00:00Z", "notes": "tests/cs16.py", "capture_drops": 0,
            "capture_drop_blocks": 0, "input_ring_drops": 0, "data_file": os.path.basename(path), "data_bytes": int(samples.nbytes)}
    with open(path + ".json", "w") as f:
        json.dump(meta, f)
    return path
