"""Inputs of the CQPSK demodulator edge tests (tests/test_oracle_cqpsk_edge.py on the CPU, tests/test_cqpsk_edge_gpu.py on the
device): the (rate, symbol rate, LPF) rows, twelve signal families that take the chain to the ends of binary32 and of its loops, and
a call plan that walks the FLL kernels' tile ring and the register kernel's chunk rotation.  Pure numpy (+ the CPU oracle for the
LPF's tap count); nothing here touches a device.

Which kernels a row launches (read from the dispatch code, ddn_dev_cqpsk_agc_fll / ddn_dev_channel_lpf_c2c in ddn_cqpsk.hip and
ddn_dev_gardner in ddn_ted.hip):
  FLL      nt = min(2 sps + 1, 48); 9, 11, 17, 21 (sps 4, 5, 8, 10) -> k_cqpsk_agc_fll_reg<nt>, every other -> k_cqpsk_agc_fll<0>
  LPF      135 taps (48 kHz) and 67 taps (24 kHz) -> k_channel_lpf_c2c_u; every other length -> k_channel_lpf_c2c
  Gardner  look-back 2 ceil(1.002 sps) <= 48, i.e. sps <= 23 -> k_gardner_ring; sps >= 24 -> k_gardner"""
import ctypes as C

import numpy as np

import orc

FAMILIES = ("subnormal", "subnormal_edge", "overflow", "silence_then_signal", "burst", "cfo_pi", "cfo_neg", "cfo1", "slow_fade",
            "real_only", "dc", "noise")
CFO = {"cfo_pi": 3.0, "cfo_neg": -0.6, "cfo1": 1.0}      # rad/sample at sps 5; scaled by 5 / sps

# (rate, symbol rate, lpf_enable, carrier-offset families whose witness the reference cannot give at this sps - named here, not skipped
# at run time; the comparison still runs them).  cfo_pi: 15 / sps rad/sample is outside what the band-edge loop pulls in on from sps 4
# up, |fll_freq| ends below 0.003 (the figures are in the table of tests/test_oracle_cqpsk_edge.py)
_PI = ("cfo_pi",)
ROWS = [
    (9600, 4800, 0, ()), (9600, 4800, 1, ()),            # sps 2, nt 5; 27-tap LPF at the fc = 0.45 fs clamp
    (14400, 4800, 0, ()), (14400, 4800, 1, ()),          # sps 3, nt 7; 41 taps
    (24000, 6000, 0, _PI), (24000, 6000, 1, _PI),        # sps 4, nt 9 (register kernel); 67 taps; the 0.018 Gardner gain
    (24000, 4800, 0, _PI), (24000, 4800, 1, _PI),        # sps 5, nt 11
    (28800, 4800, 0, _PI), (28800, 4800, 1, _PI),        # sps 6, nt 13; 81 taps
    (38400, 4800, 1, _PI),                               # sps 8, nt 17; 107 taps
    (48000, 6000, 1, _PI),                               # sps 8, 135 taps, 6000 sym/s
    (48000, 4800, 1, _PI),                               # sps 10, nt 21
    (96000, 4800, 0, _PI),                               # sps 20, nt 41
    (115200, 4800, 0, _PI),                              # sps 24: the tap cap 49 -> 48, the first classic-Gardner sps
    (120000, 4800, 0, _PI),                              # sps 25
]
# sample rates that are no multiple of the symbol rate: the Gardner stage's gain goes by (rate + sps / 2) / sps, as the reference's
# (rate, symbol rate, a whole-ratio rate of the same sps whose derived symbol rate stays below 5500 = the gain held, switches?)
NONINT_ROWS = [(12000, 4800, 9600, True), (28000, 4800, 24000, True), (26000, 4800, 24000, False)]

REG_NT = (9, 11, 17, 21)


def row_id(row):
    return "%d-%d-lpf%d" % row[:3]


def block_len(rate):
    return 333 if rate <= 28800 else 1000


def n_symbols(sps):
    """symbols per stream: 700; 1000 at sps 2, where 700 symbols are fewer samples than the call plan's fixed groups; 1500 from sps 8 up,
    where the Gardner and Costas loops need more than 700 symbols to lock (on the plain signal too) - a row whose loops never converge
    would compare the kernels on an unlocked chain only"""
    return 1000 if sps == 2 else (1500 if sps >= 8 else 700)


def fll_taps(sps):
    return min(2 * sps + 1, 48)


def lpf_taps(rate, lpf, profile=5):
    if not lpf:
        return 0
    buf = (C.c_float * 144)()
    n = orc.oracle().orc_channel_lpf_design(rate, profile, buf, 144)
    assert n >= 3, (rate, n)
    return n


def family(name, sps, n_sym=700, seed=0):
    """one float32 [n][2] stream, n = n_sym * sps - 40"""
    def base(**k):
        return orc.synth_dqpsk_f32(seed, 1, n_sym, sps, **k)[0]
    if name == "subnormal":                 # |x|^2 a few ulps of 2^-149: the mean square ends subnormal
        return base() * np.float32(1e-22)
    if name == "subnormal_edge":            # |x|^2 about 2^-126: the mean square straddles the smallest normal
        return base() * np.float32(2e-19)
    if name == "overflow":                  # |x|^2 = +inf: gain 0 from the first sample on, agc_avg stays inf
        return base() * np.float32(1e20)
    if name == "silence_then_signal":       # the mean square decays to 2^-149, then a whisper and the signal meet enormous gains
        x = base()
        x[40 * sps:190 * sps] = 0
        x[190 * sps:210 * sps] *= np.float32(1e-6)
        return x
    if name == "burst":                     # ten samples whose |x|^2 is near the top of binary32 without reaching inf
        x = base()
        x[60 * sps:60 * sps + 10] *= np.float32(1e19)
        return x
    if name in CFO:                         # a real carrier offset: NCO phase wraps at +-2 pi, every quadrant of sincos_two_pi
        return base(cfo=CFO[name] * 5.0 / sps, noise=0.3 if name == "cfo1" else 0.03)
    if name == "slow_fade":                 # down to 1 % and back: Costas confidence 0, the smoothstep band, es reset
        x = base()
        n = len(x)
        ramp = np.concatenate([np.linspace(1, 0.01, n // 2), np.linspace(0.01, 1, n - n // 2)]).astype(np.float32)
        return x * ramp[:, None]
    if name == "real_only":
        x = base()
        x[:, 1] = 0
        return x
    if name == "dc":
        x = base()
        x[:] = np.float32(0.3)
        return x
    if name == "noise":
        return (np.random.default_rng(seed).standard_normal((n_sym * sps - 40, 2)) * 0.3).astype(np.float32)
    raise KeyError(name)


def families(sps, n_sym=700, seed=0):
    return {name: family(name, sps, n_sym, seed) for name in FAMILIES}


def call_plan(n, sps, blk, taps_len):
    """call lengths for a stream of n samples (their sum = the prefix of n the plan uses): (1) twelve calls cycling 4, 5, 6, 7 - shorter
    than a chunk; (2) NT + r for every r in 0 .. NT - 1 in a seeded shuffle - a whole chunk and every tail, every rotation of the stored
    delay line, each followed by a different one; (3) TS - 1, TS, TS + 1, 2 TS, 2 TS + 1, 3 TS + 1 - the three-tile ring through
    stage-without-prefetch, the first wrap, drain-after-loop; (4) with the LPF: blk + 4 (the shortest legal ragged block), blk + taps_len
    - 1 and blk + taps_len (the (mul, add) and the FMA side of the ragged block); (5) the rest in one call."""
    NT = fll_taps(sps)
    TS = 3 * NT if NT in REG_NT else 32
    plan = [4 + k % 4 for k in range(12)]
    plan += [NT + int(r) for r in np.random.default_rng(NT).permutation(NT)]
    plan += [TS - 1, TS, TS + 1, 2 * TS, 2 * TS + 1, 3 * TS + 1]
    if taps_len:
        plan += [blk + 4, blk + taps_len - 1, blk + taps_len]
    rest = n - sum(plan)
    assert rest >= 0, (n, sum(plan))
    rest -= rest % blk if rest % blk < 4 else 0     # the plan uses a prefix of the stream
    if rest >= 4:
        plan.append(rest)
    # a block of 1-3 samples leaves the reference's Gardner stage without output (ddn_cqpsk_run rejects such a call)
    assert all(L >= 4 and not 1 <= L % blk <= 3 for L in plan), plan
    return plan


def watched_calls(sps):
    """the calls of groups 1 and 2 of call_plan: the device test compares the carried state after each of them"""
    return 12 + fll_taps(sps)


def channel_stream(c, sps, n_sym):
    """channel c of the device test: family c % 12 with seed c; channels 12-23 negated, 24 and up with I and Q swapped"""
    x = family(FAMILIES[c % 12], sps, n_sym, seed=c)
    if 12 <= c < 24:
        x = -x
    elif c >= 24:
        x = np.ascontiguousarray(x[:, ::-1])
    return x
