"""The analog FM monitor's checkers: the CPU restatement of full_demod()'s audio output kind (tests/fm_audio_ref.c, built here against
the oracle's exported helpers), the driver around the compiled reference (tests/fm_audio_refdrv.cpp, built where the reference's headers
and oracle/_ref exist), the configurations the tests walk and the seeded inputs.  TEST INFRASTRUCTURE."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 1024
STATE_NAMES = ("pre_r", "pre_j", "deemph_avg", "audio_lpf_state", "dc_avg", "now_lpr", "squelch_env", "gate")

# what a configuration may set; every test names only what it changes
DEFAULTS = dict(rate=48000, profile=0, passes=0, M=1, deemph=1, tau=0, lpf=0, dc=1, lpr=None, squelch=0.0, attack=0.0, release=0.0)

PASSES = (0, 1, 2)
DECIMS = (1, 2, 3, 5)
LPRS = ((48000, 48000), (96000, 48000), (48000, 8000), (48000, 32000), None)

# the six configurations of tests/golden/fm_audio_*.npz
GOLDEN = {
    "nfm_default": dict(),
    "analog_p1_lpr": dict(passes=1, lpr=(96000, 48000)),
    "decim3_lpr8k": dict(M=3, lpr=(48000, 8000), tau=750),
    "decim5_p2_lpf": dict(passes=2, M=5, lpf=3000, tau=50, lpr=(48000, 32000)),
    "squelch_mid": dict(squelch=0.02, M=2, lpr=(48000, 48000)),
    "all_off": dict(deemph=0, dc=0, M=2),
}


def cfg(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def configs():
    """name -> configuration: every configuration the GPU tests walk (the oracle test pins the restatement on each of them)"""
    out = {}
    for p in PASSES:
        for M in DECIMS:
            out["p%d_M%d" % (p, M)] = cfg(passes=p, M=M)
    for lpr in LPRS:
        for M in (1, 3):
            out["lpr_%s_M%d" % ("off" if lpr is None else "%d_%d" % lpr, M)] = cfg(lpr=lpr, M=M)
    for deemph in (0, 1):
        for lpf in (0, 3000):
            for dc in (0, 1):
                out["sw_d%d_l%d_c%d" % (deemph, lpf, dc)] = cfg(deemph=deemph, lpf=lpf, dc=dc)
    for tau in (50, 75, 750):
        out["tau%d" % tau] = cfg(tau=tau)
    out["squelch_above"] = cfg(squelch=1.0, M=2)
    out["squelch_below"] = cfg(squelch=1.0e-6)
    out["squelch_mid"] = cfg(squelch=0.02, M=3, lpr=(48000, 32000), lpf=3000)
    out["squelch_mid_env"] = cfg(squelch=0.02, attack=0.5, release=0.25, passes=1)
    return out


OCCO = [0.6, 0.04, 0.04, 0.6]   # carrier amplitude per block: open, closed, closed, open under a squelch level of 0.02


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """bit for bit; two NaNs at the same place count as equal whatever their payloads"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def _icfg(c):
    fast, slow = c["lpr"] if c["lpr"] else (0, 0)
    return (C.c_int * 10)(c["rate"], c["profile"], c["passes"], c["M"], c["deemph"], c["tau"], c["lpf"], c["dc"], fast, slow)


def _fcfg(c):
    return (C.c_float * 3)(c["squelch"], c["attack"], c["release"])


def _build(src, tag_extra, cmd_of):
    tag = hashlib.sha1(open(src, "rb").read() + tag_extra).hexdigest()[:12]
    so = os.path.join(tempfile.gettempdir(), "ddn_%s_%d_%s.so" % (os.path.basename(src).split(".")[0], os.getuid(), tag))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call(cmd_of(tmp))
        os.replace(tmp, so)
    return C.CDLL(so)


_RST = None


def restatement():
    global _RST
    if _RST is None:
        orc.oracle()                                    # (builds oracle/libddn_oracle.so where it is missing)
        src = os.path.join(HERE, "fm_audio_ref.c")
        odir = os.path.join(orc.ROOT, "oracle")
        l = _build(src, open(orc.ORACLE_SO, "rb").read(),
                   lambda out: ["gcc", "-std=c11", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", odir,
                                src, orc.ORACLE_SO, "-lm", "-Wl,-rpath," + odir, "-o", out])
        l.fmr_sizeof.restype = C.c_size_t
        l.fmr_init.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.fmr_run.restype = C.c_long
        l.fmr_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
        l.fmr_get_state.argtypes = [C.c_void_p, C.c_void_p]
        l.fmr_get_phases.argtypes = [C.c_void_p, C.c_void_p]
        l.fmr_get_coefficients.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.fmr_set_coefficients.argtypes = [C.c_void_p, C.c_float, C.c_float]
        _RST = l
    return _RST


def _fmt_of(iq):
    return {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.int16): 2}[iq.dtype]


class Restatement:
    """one channel of the restatement; run(iq [n, 2] uint8 / float32 / int16) -> float32 [count], state carried across calls"""

    def __init__(self, c, block_len=BLOCK):
        self.l = restatement()
        self.c, self.block_len = c, block_len
        self.st = C.create_string_buffer(self.l.fmr_sizeof())
        assert self.l.fmr_init(self.st, _icfg(c), _fcfg(c)) >= 3

    def run(self, iq):
        iq = np.ascontiguousarray(iq)
        n = iq.shape[0]
        out = np.zeros(max(1, n), np.float32)
        k = self.l.fmr_run(self.st, _fmt_of(iq), iq.ctypes.data, n, self.block_len, out.ctypes.data)
        if k < 0:
            raise ValueError("a block without a decimator output: the reference keeps it un-decimated, not restated")
        return out[:k].copy()

    def state(self):
        s = np.zeros(8, np.float32)
        self.l.fmr_get_state(self.st, s.ctypes.data)
        return s

    def phases(self):
        p = np.zeros(2, np.int32)
        self.l.fmr_get_phases(self.st, p.ctypes.data)
        return int(p[0]), int(p[1])

    def coefficients(self):
        c3, t16 = np.zeros(3, np.float32), np.zeros(16, np.float32)
        self.l.fmr_get_coefficients(self.st, c3.ctypes.data, t16.ctypes.data)
        return c3, t16

    def set_coefficients(self, deemph_a, lpf_alpha):
        self.l.fmr_set_coefficients(self.st, deemph_a, lpf_alpha)


def restate_batch(c, iq, calls=None, block_len=BLOCK):
    """iq [B, n, 2]; calls = the lengths of consecutive calls (None: one) -> (audio [B, count], states [B, 8])"""
    B, n = iq.shape[0], iq.shape[1]
    calls = calls or [n]
    assert sum(calls) == n
    rows, states = [], []
    for ch in range(B):
        r = Restatement(c, block_len)
        parts, pos = [], 0
        for m in calls:
            parts.append(r.run(iq[ch, pos:pos + m]))
            pos += m
        rows.append(np.concatenate(parts))
        states.append(r.state())
    return np.stack(rows), np.stack(states)


# ---- the compiled reference ------------------------------------------------------------------------------------------------------
def have_reference():
    return orc.have_ref() and os.path.isdir(os.path.join(orc.REFERENCE_ROOT, "include", "dsd-neo"))


_DRV = None


def driver():
    global _DRV
    if _DRV is None:
        src = os.path.join(HERE, "fm_audio_refdrv.cpp")
        ref = orc.REFERENCE_ROOT
        rdir = os.path.dirname(orc.REF_SO)
        # the definitions oracle/Makefile compiles the reference with: they decide struct demod_state's layout
        l = _build(src, open(orc.REF_SO, "rb").read(),
                   lambda out: ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-DUSE_RADIO", "-DDSD_NEO_DSP_HAVE_AVX2_IMPL=1", "-D_GNU_SOURCE",
                                "-I", os.path.join(ref, "include"), "-I", os.path.join(ref, "src", "dsp"), src, orc.REF_SO,
                                "-Wl,-rpath," + rdir, "-o", out])
        l.fmdrv_create.restype = C.c_void_p
        l.fmdrv_create.argtypes = [C.c_void_p, C.c_void_p]
        l.fmdrv_destroy.argtypes = [C.c_void_p]
        l.fmdrv_run.restype = C.c_long
        l.fmdrv_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
        l.fmdrv_state.argtypes = [C.c_void_p, C.c_void_p]
        l.fmdrv_phases.argtypes = [C.c_void_p, C.c_void_p]
        l.fmdrv_taps.argtypes = [C.c_void_p, C.c_void_p]
        _DRV = l
    return _DRV


class Reference:
    """one demod_state of the compiled reference in the audio-monitor kind.  The two coefficients the reference derives outside the
    units built here (rtl_sdr_fm.cpp) come from the restatement's design; cs16 is fed as the exact floats it widens to."""

    def __init__(self, c, block_len=BLOCK):
        self.l = driver()
        self.block_len = block_len
        c3, _ = Restatement(c).coefficients()
        ic = _icfg(c)
        ic[6] = 1 if c["lpf"] > 0 else 0
        fc = (C.c_float * 5)(c["squelch"], c["attack"], c["release"], c3[0], c3[1])
        self.h = self.l.fmdrv_create(ic, fc)
        assert self.h

    def run(self, iq):
        iq = np.ascontiguousarray(iq)
        if iq.dtype == np.int16:
            iq = iq.astype(np.float32) * np.float32(1.0 / 32768.0)
        n = iq.shape[0]
        out = np.zeros(max(1, n), np.float32)
        k = self.l.fmdrv_run(self.h, _fmt_of(iq), iq.ctypes.data, n, self.block_len, out.ctypes.data)
        return out[:k].copy()

    def state(self):
        s = np.zeros(8, np.float32)
        self.l.fmdrv_state(self.h, s.ctypes.data)
        return s

    def phases(self):
        p = np.zeros(2, np.int32)
        self.l.fmdrv_phases(self.h, p.ctypes.data)
        return int(p[0]), int(p[1])

    def taps(self):
        t = np.zeros(16, np.float32)
        return t if self.l.fmdrv_taps(self.h, t.ctypes.data) == 16 else None

    def close(self):
        if self.h:
            self.l.fmdrv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def synth_nfm(seed, n_ch, n, rate=48000, amp=0.6, noise=0.02, fmt="cu8", amp_blocks=None, block_len=BLOCK):
    """narrow-band FM of a two-tone audio signal, a small carrier offset per channel, additive noise -> [n_ch, n, 2] cu8 / cs16 / cf32.
    amp_blocks: the carrier's amplitude per block of block_len samples (the last one repeats), for runs through the squelch gate"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    if amp_blocks is not None:
        k = np.minimum(np.arange(n) // block_len, len(amp_blocks) - 1)
        amp = np.asarray(amp_blocks, np.float64)[k]
    out = np.empty((n_ch, n, 2), np.float64)
    for c in range(n_ch):
        f1, f2 = 400.0 + 170.0 * c + 50.0 * rng.random(), 1300.0 + 90.0 * c
        audio = 0.7 * np.sin(2 * np.pi * f1 * t + rng.random()) + 0.3 * np.sin(2 * np.pi * f2 * t)
        ph = 2 * np.pi * np.cumsum(2500.0 * audio + 300.0 * (c - n_ch / 2.0)) / rate + 6.28 * rng.random()
        out[c, :, 0] = amp * np.cos(ph) + noise * rng.standard_normal(n)
        out[c, :, 1] = amp * np.sin(ph) + noise * rng.standard_normal(n)
    return quantise(out, fmt)


def quantise(x, fmt):
    if fmt == "cu8":
        return np.clip(np.rint(127.5 + 127.5 * x), 0, 255).astype(np.uint8)
    if fmt == "cs16":
        return np.clip(np.rint(32768.0 * x), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def widen(iq):
    """the floats a cu8 / cs16 array widens to on every path (exact in binary32)"""
    if iq.dtype == np.uint8:
        return ((iq.astype(np.float32) - np.float32(127.5)) * (np.float32(1.0) / np.float32(127.5))).astype(np.float32)
    if iq.dtype == np.int16:
        return iq.astype(np.float32) * np.float32(1.0 / 32768.0)
    return iq


def golden_path(name):
    return os.path.join(HERE, "golden", "fm_audio_%s.npz" % name)


GOLDEN_N = 2400
GOLDEN_CALLS = [1024, 600, 776]   # call boundaries = block boundaries of the recorded run: multiples of 4, every tail >= 5 after 2 passes
GOLDEN_AMPS = [0.6, 0.04, 0.6]    # the middle block falls below squelch_mid's level


# ---- the device side -------------------------------------------------------------------------------------------------------------
def make_batch(ddn, c, n_channels, input_format, block_len=BLOCK):
    kw = dict(post_downsample=c["M"], deemph=c["deemph"], deemph_tau_us=c["tau"], audio_lpf_cutoff_hz=c["lpf"], dc_block_off=0 if c["dc"] else 1,
              squelch_env_attack=c["attack"], squelch_env_release=c["release"])
    if c["lpr"]:
        kw.update(lpr_fast_hz=c["lpr"][0], lpr_slow_hz=c["lpr"][1])
    return ddn.FmAudio(n_channels, sample_rate_hz=c["rate"], lpf_profile=c["profile"], input_format=input_format, block_len=block_len,
                       squelch_level=c["squelch"], passes=c["passes"], **kw)


def device_batch(ddn, c, iq, calls=None, block_len=BLOCK):
    """the same run as restate_batch on the device -> (audio [B, count], states [B, 8])"""
    fmt = {np.dtype(np.uint8): ddn.IN_CU8, np.dtype(np.float32): ddn.IN_CF32, np.dtype(np.int16): ddn.IN_CS16}[iq.dtype]
    B, n = iq.shape[0], iq.shape[1]
    calls = calls or [n]
    b = make_batch(ddn, c, B, fmt, block_len)
    parts, pos = [], 0
    for m in calls:
        parts.append(b.run_host(np.ascontiguousarray(iq[:, pos:pos + m]), m))
        pos += m
    st = np.stack([b.audio_state(ch) for ch in range(B)])
    b.close()
    return np.concatenate(parts, axis=1), st
