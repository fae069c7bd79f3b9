"""Float64 model of the vocoder's enhancement, phase track and synthesis.  TEST INFRASTRUCTURE, numpy only.

Written from the equations of the mbelib lineage that the product cites (mbe_spectralAmpEnhance, mbe_synthesizeSpeechf at
unvoiced quality 3) and shares no code with oracle/ or with the product.  Inputs are binary32 state values; every operation
after that is float64 with np.cos / np.exp / np.sqrt.  Every constant the product writes as a `float` literal is taken at
its binary32 value (UVSTEP, UVOFFSET, UVSINE, QFACTOR, UVTHRESHOLD, pi, 2 pi, 0.96, 0.693, 0.2046), so that what remains
between this model and the product is rounding and the two polynomials alone.  The hash that replaced rand() is integer work
and is reproduced exactly in uint32.

Why 2^-14 * A[n] + 2^-20 bounds |pcm[n] - synth(...)[n]| (derived, not measured).  A[n] is the sum of the absolute
amplitudes of every term of sample n, so the bound is a bound on the relative error of ONE term, eps_term, plus what the
accumulation adds.  Harmonic l of a side with fundamental w0 has l * w0 < pi, and |n|, |n - 160| <= 160, so a cosine argument
is below 161 pi < 512.  Per term, in units of the term's amplitude (|d cos| <= |d argument|):
  * the product (w0 l) n and the sum with the phase each round at half an ulp of [256, 512) = 2^-16          3.05e-5
    (together; the unvoiced argument (w0 n)(l + i/3 - 1/3) + phase has the same two final roundings)
  * the rounding of w0 l (or w0 n, or l + i/3 - 1/3) at 2^-24 relative, carried to an argument below 512:
    512 * 2^-24 = 2^-15 is the worst case at the far end of the frame, half of that at the argument's mean
    over the frame                                                                                          1.5e-5 .. 3.05e-5
  * the cosine polynomial (measured against double cos, tests/test_mbe_ref64.py)                              1e-7
  * three products (window, amplitude, the unvoiced scale factors) at 2^-24                                   1.8e-7
  * the hashed phase u * 2pi - pi: two roundings at 2^-24 of a value below 2 pi                               7.5e-7
  * the accumulation of at most 57 terms: each partial sum is below A[n], 57 * 2^-24 * A[n]                    3.4e-6
The sum is 5.0e-5 with the mean carry and 6.5e-5 with every rounding at its extreme at the frame's far end; the bound is
2^-14 = 6.1e-5: the extreme needs four independent roundings to be maximal and of one sign on the dominant term, at the last
sample of a harmonic whose l * w0 is next to pi.  The absolute 2^-20 only covers samples where A[n] is itself zero or subnormal.  Measured worst cases are written in
the tests' docstrings.
"""
import numpy as np

_F = lambda v: float(np.float32(v))
PI = _F(3.14159265358979323846)
TWO_PI = _F(6.28318530717958647692)
UVTHRESHOLD = _F(2.12057504117311)      # 2700 pi / 4000
UVSINE = _F(3.69452831983566)           # 1.3591409 e
UVRAND = 2.0
UVSTEP = _F(0.333333333333333)          # 1 / uvquality
UVOFFSET = _F(0.333333333333333)        # uvstep (uvquality - 1) / 2
QFACTOR = _F(0.366204096222703)         # log(3) / 3
C096 = _F(0.96)
C0693 = _F(0.693)
C02046 = _F(0.2046)
N = 160
LMAX = 56
IMBE, AMBE = 0, 1
_M32 = np.uint64(0xFFFFFFFF)


class Side:
    """one side of the cross-fade: fundamental, harmonic count, and per harmonic l = 0..56 voicing, amplitude, phases (binary32
    values held as float64).  Side.of(p) takes anything with the fields of an mbe_parms."""

    def __init__(self, w0, L, V, M, PHI=None, PSI=None):
        self.w0, self.L = float(np.float32(w0)), int(L)
        self.V = np.asarray(V, np.int64).copy()
        self.M = np.asarray(M, np.float32).astype(np.float64)
        self.PHI = np.zeros(57) if PHI is None else np.asarray(PHI, np.float32).astype(np.float64)
        self.PSI = np.zeros(57) if PSI is None else np.asarray(PSI, np.float32).astype(np.float64)

    @classmethod
    def of(cls, p):
        return cls(p.w0, p.L, p.Vl[:], p.Ml[:], p.PHIl[:], p.PSIl[:])


def mix(h, v):
    h = (np.asarray(h, np.uint64) ^ np.asarray(v, np.uint64)) & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & _M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & _M32
    h ^= h >> np.uint64(16)
    return h


def u01(h):
    return (np.asarray(h, np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def rand_phase(h):
    return u01(h) * TWO_PI - PI


def frame_key(seed, frame_no):
    return mix(mix(0x9E3779B9, int(seed) & 0xFFFFFFFF), int(frame_no) & 0xFFFFFFFF)


def window(t):
    """synthesis window at time t from a frame's centre: 1 within +-55, 0 from +-105 on, linear in between"""
    a = np.abs(np.asarray(t, np.float64))
    return np.clip((105.0 - a) / 50.0, 0.0, 1.0)


def _unvoiced(w0, l, n, base, tag):
    """sum of the three hashed-phase cosines and, above the threshold, the hashed noise: [l][n]"""
    w0l = w0 * l
    c3 = np.zeros((l.size, n.size))
    over = np.maximum(w0l - UVTHRESHOLD, 0.0)
    for i in range(3):
        rph = rand_phase(mix(base, tag + i))
        c3 += np.cos((w0 * n)[None, :] * ((l + i * UVSTEP) - UVOFFSET)[:, None] + rph[:, None])
        noise = u01(mix(mix(base, tag + 0x40 + i)[:, None], n.astype(np.uint64)[None, :]))
        c3 += (over * UVRAND)[:, None] * noise
    return c3


def synth(prev_side, cur_side, seed, frame_no, window_shift=0, cur_origin=N, phi_sign=1.0):
    """-> (pcm[160], A[160]).  The keyword arguments exist for the mutation checks only."""
    l = np.arange(1, LMAX + 1, dtype=np.float64)
    li = np.arange(1, LMAX + 1)
    n = np.arange(N, dtype=np.float64)
    base = mix(frame_key(seed, frame_no), li.astype(np.uint64))
    pcm = np.zeros(N)
    A = np.zeros(N)
    # (side, time from the side's frame centre in the window, time in the voiced oscillator, hash tag of the unvoiced bank)
    for side, tw, t, tag in ((prev_side, n, n, 0x300), (cur_side, n - N, n - cur_origin, 0x200)):
        live = li <= side.L                               # a harmonic above a side's L has amplitude 0
        M = np.where(live, side.M[1:], 0.0)
        voiced = np.where(live, side.V[1:] != 0, True)
        w = window(tw + window_shift)
        vo = np.cos(side.w0 * l[:, None] * t[None, :] + phi_sign * side.PHI[1:, None])
        uv = np.zeros_like(vo)
        rows = np.flatnonzero(~voiced & (M != 0.0))       # the unvoiced bank only where it is heard
        if rows.size:
            uv[rows] = _unvoiced(side.w0, l[rows], n, base[rows], tag) * UVSINE * QFACTOR
        pcm += (np.where(voiced[:, None], vo, uv) * M[:, None]).sum(axis=0) * w
        amp = np.where(voiced, 1.0, UVSINE * QFACTOR * (3.0 + 3.0 * UVRAND * np.maximum(side.w0 * l - UVTHRESHOLD, 0.0)))
        A += np.sum(np.abs(M) * amp) * w
    return pcm, A


def enhance(w0, L, Ml, clamp_hi=1.2, details=False):
    """spectral amplitude enhancement of Ml[1..L] (Ml is indexed by harmonic, [0] unused) -> Ml' of the same shape.
    details=True also returns (cancel[57], W[57]): cancel[l] is how far the harmonic's x = num / den is from an exact 0 / 0 -
    the smaller of |num| and |den| relative to the sum of their terms' absolute values (tests skip a harmonic below 2^-18)."""
    w0 = float(np.float32(w0))
    M = np.asarray(Ml, np.float32).astype(np.float64)
    out = M.copy()
    l = np.arange(1, L + 1)
    m = M[1:L + 1]
    c = np.cos(w0 * l)
    Rm0, Rm1 = np.sum(m * m), np.sum(m * m * c)
    R2m0, R2m1 = Rm0 * Rm0, Rm1 * Rm1
    cross = 2.0 * Rm0 * Rm1 * c
    with np.errstate(all="ignore"):
        num = C096 * PI * ((R2m0 + R2m1) - cross)
        den = w0 * Rm0 * (R2m0 - R2m1)
        x = num / den
        tmp = np.sqrt(m) * np.sqrt(np.sqrt(x))
        exempt = (8 * l <= L) | (m == 0.0) | ~(x > 0.0) | ~np.isfinite(x)
        W = np.where(exempt, 1.0, np.clip(np.where(exempt, 1.0, tmp), 0.5, clamp_hi))
        me = m * W
        s = np.sum(me * me)
        gamma = 1.0 if s == 0.0 else np.sqrt(Rm0 / s)
        out[1:L + 1] = gamma * me
        if not details:
            return out
        cancel = np.ones(57)
        cn = np.abs((R2m0 + R2m1) - cross) / (R2m0 + R2m1 + np.abs(cross))
        cd = np.full(L, abs(R2m0 - R2m1) / (R2m0 + R2m1))
        cancel[1:L + 1] = np.where(m == 0.0, 1.0, np.nan_to_num(np.minimum(cn, cd), nan=0.0))
        Wd = np.ones(57)
        Wd[1:L + 1] = W
    return out, cancel, Wd


def phases(prev_enh, cur, num_uv, seed, frame_no, half=N // 2):
    """phase track of one frame: prev_enh carries PSIl and w0 of the previous frame, cur w0 and L of this one.
    -> (PSIl[57], PHIl[57]), unwrapped (compare modulo 2 pi); [0] unused"""
    l = np.arange(57)
    psi = prev_enh.PSI + (prev_enh.w0 + cur.w0) * l * float(half)
    dither = rand_phase(mix(mix(frame_key(seed, frame_no), l.astype(np.uint64)), 0x100))
    phi = np.where(l <= cur.L // 4, psi, psi + num_uv * dither / cur.L)
    psi[0] = phi[0] = 0.0
    return psi, phi


def ml_from_log2(log2Ml, voiced, w0, codec):
    x = np.asarray(log2Ml, np.float32).astype(np.float64)
    m = np.exp(C0693 * x)
    if codec == AMBE:
        m = np.where(np.asarray(voiced) != 0, m, m * (C02046 / np.sqrt(float(np.float32(w0)))))
    return m


def circ(a, b):
    """|a - b| modulo 2 pi"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs(d - 2.0 * np.pi * np.rint(d / (2.0 * np.pi)))
