"""CPU: the vocoder restatement (oracle/ddn_oracle_mbe.c) held to the float64 model of tests/mbe_ref64.py, the mutation
checks that prove the bounds can fail, the product's and the restatement's elementary functions against double libm and
against each other, and the statistics of the hash that replaced rand().

The cases, the drivers and the checks of this file are shared with tests/test_mbe_ref64_gpu.py, which runs them on the device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ddn
import mbe
import mbe_ref64 as R

CODECS = [ddn.MBE_IMBE, ddn.MBE_AMBE]
B_SYNTH, B_ABS = 2.0 ** -14, 2.0 ** -20      # |pcm - ref| <= B_SYNTH * A + B_ABS
B_ENH = 2.0 ** -18                           # enhanced amplitude, relative; energy, relative; also the skip threshold
B_PHASE = 2.0 ** -11                         # PSIl / PHIl, circular, rad
B_ML = 2.0 ** -20                            # Ml against exp(0.693 log2Ml), relative
PI32 = np.float32(R.PI)
REPEAT, MUTE = 0x8, 0x10
FIRST_STREAM = 0x12345


# ---- chosen states --------------------------------------------------------------------------------------------------
def parms(w0, L, V, M, PHI=None, PSI=None, un=0, repeat=0):
    p = ddn.MbeParms()
    p.w0, p.L, p.K = float(np.float32(w0)), int(L), (int(L) + 2) // 3 if L < 37 else 12
    z = np.zeros(57, np.float32)
    for name, v in (("Ml", M), ("PHIl", z if PHI is None else PHI), ("PSIl", z if PSI is None else PSI)):
        setattr(p, name, (C.c_float * 57)(*[float(x) for x in np.asarray(v, np.float32)]))
    p.Vl = (C.c_int * 57)(*[int(x) for x in V])
    p.un, p.repeat = int(np.int32(np.uint32(un))), repeat
    return p


def clone(p):
    return ddn.MbeParms.from_buffer_copy(bytes(p))


def w0_of(L):
    """a fundamental that fits L harmonics below pi, as the codecs' own (w0, L) pairs do"""
    return np.float32(np.pi / (L + 1.25))


def _voicing(kind, L, rng):
    l = np.arange(57)
    v = {"v": np.ones(57, int), "u": np.zeros(57, int), "alt": l & 1, "alt2": 1 - (l & 1), "rnd": rng.integers(0, 2, 57)}[kind]
    v = v.copy()
    v[L + 1:] = rng.integers(0, 2, 56 - L)      # whatever a shorter earlier frame left above L must not matter
    return v


def _amps(L, rng, junk=True):
    m = np.zeros(57, np.float32)
    m[1:L + 1] = np.exp(rng.uniform(-2.0, 3.0, L))
    if junk:
        m[L + 1:] = np.exp(rng.uniform(0.0, 3.0, 56 - L))
    return m


def build_cases(seed=20240611):
    """about 96 talk paths: each a dict cur = (w0, L, V, M) of the frame to be repeated (un-enhanced), prev = (w0, L, V, M, PHI, PSI) of
    the enhanced previous frame, frame_no"""
    rng = np.random.default_rng(seed)
    cases = []
    frames = [0, 1, 2 ** 31 - 1, 77, 123456789]

    def add(name, Lp, Lc, vp, vc, wp=None, wc=None, edit=None):
        c = {"name": name, "frame_no": frames[len(cases) % len(frames)],
             "prev": [w0_of(Lp) if wp is None else np.float32(wp), Lp, _voicing(vp, Lp, rng), _amps(Lp, rng),
                      rng.uniform(-np.pi, np.pi, 57).astype(np.float32), rng.uniform(-np.pi, np.pi, 57).astype(np.float32)],
             "cur": [w0_of(Lc) if wc is None else np.float32(wc), Lc, _voicing(vc, Lc, rng), _amps(Lc, rng)]}
        if edit:
            edit(c)
        cases.append(c)

    partner = {9: 13, 10: 36, 12: 9, 13: 56, 36: 10, 37: 55, 55: 37, 56: 12}
    # voicing pairs (previous side, current side): all voiced, all unvoiced, alternating, voiced against unvoiced on the same
    # harmonic in both directions (whole spectrum and harmonic by harmonic), random
    pairs = [("v", "v"), ("u", "u"), ("alt", "alt"), ("v", "u"), ("u", "v"), ("alt", "alt2"), ("alt2", "alt"), ("rnd", "rnd"), ("rnd", "v")]
    k = 0
    for L in (9, 10, 12, 13, 36, 37, 55, 56):
        for Lp, Lc in ((L, L), (L, partner[L]), (partner[L], L)):
            for _ in range(3):
                vp, vc = pairs[k % len(pairs)]
                k += 1
                add("L%d/%d %s/%s" % (Lp, Lc, vp, vc), Lp, Lc, vp, vc)
    # harmonic 38 of a 55-harmonic frame just below and just above UVTHRESHOLD (the noise term switches on there)
    for eps in (-2.0 ** -18, 2.0 ** -18, -2.0 ** -10, 2.0 ** -10):
        w = R.UVTHRESHOLD * (1.0 + eps) / 38.0
        add("threshold %+g" % eps, 55, 55, "u", "u", wp=w, wc=w)
    add("threshold mixed", 56, 55, "alt", "alt2", wp=np.pi / 56.3, wc=np.pi / 55.4)
    add("threshold rnd", 43, 56, "rnd", "u", wp=np.pi / 43.3, wc=np.pi / 56.2)

    def zero(side, which):
        def f(c):
            L = c[side][1]
            idx = np.arange(1, L + 1) if which == "all" else np.arange(1, L + 1)[which::3]
            c[side][3][idx] = 0.0
        return f

    def both(*fs):
        def f(c):
            for g in fs:
                g(c)
        return f
    add("zeros cur", 37, 36, "rnd", "rnd", edit=zero("cur", 0))
    add("zeros prev", 36, 37, "alt", "rnd", edit=zero("prev", 1))
    add("zeros both same", 37, 37, "rnd", "alt", edit=both(zero("cur", 2), zero("prev", 2)))
    add("zeros both other", 13, 12, "u", "v", edit=both(zero("cur", 0), zero("prev", 1)))
    add("prev all zero", 36, 13, "rnd", "rnd", edit=zero("prev", "all"))
    add("cur all zero", 13, 36, "rnd", "rnd", edit=zero("cur", "all"))
    add("both all zero", 12, 55, "rnd", "rnd", edit=both(zero("cur", "all"), zero("prev", "all")))

    def dominant(side, l, voiced):
        def f(c):
            L = c[side][1]
            c[side][3][1:L + 1] = 1.0
            c[side][3][l] = 1.0e4
            c[side][2][l] = voiced
        return f
    add("dominant prev voiced", 13, 13, "v", "v", edit=dominant("prev", 5, 1))
    add("dominant cur voiced", 37, 37, "v", "alt", edit=dominant("cur", 20, 1))
    add("dominant prev unvoiced", 36, 12, "u", "v", edit=dominant("prev", 30, 0))
    add("dominant cur unvoiced", 12, 56, "alt", "u", edit=dominant("cur", 50, 0))
    add("dominant both", 56, 56, "v", "v", edit=both(dominant("cur", 56, 1), dominant("prev", 1, 1)))

    def phase(v):
        def f(c):
            c["prev"][4][:] = v
            c["prev"][5][:] = v
        return f
    add("phase +pi", 37, 36, "v", "v", edit=phase(PI32))
    add("phase -pi", 12, 13, "alt", "alt", edit=phase(-PI32))

    def phase_alternating(c):
        phase(PI32)(c)
        c["prev"][4][::2] = -PI32
    add("phase +-pi", 55, 56, "v", "rnd", edit=phase_alternating)
    while len(cases) < 96:
        Lp, Lc = int(rng.integers(9, 57)), int(rng.integers(9, 57))
        vp, vc = pairs[int(rng.integers(len(pairs)))]
        add("random L%d/%d %s/%s" % (Lp, Lc, vp, vc), Lp, Lc, vp, vc)
    for c in cases:
        for side in ("prev", "cur"):
            assert c[side][0] * c[side][1] < np.pi          # l w0 < pi, as in every frame either codec can decode
    return cases


def case_triple(c):
    """{cur, prev, prev_enhanced} as set before the repeat frame"""
    w0, L, V, M = c["cur"]
    prev = parms(w0, L, V, M, un=c["frame_no"])
    pw0, pL, pV, pM, pPHI, pPSI = c["prev"]
    enh = parms(pw0, pL, pV, pM, pPHI, pPSI, un=c["frame_no"])
    return clone(prev), prev, enh


def repeat_frames(codec, S, F=1, seed=5):
    """ordinary parameter bits whose frame decode reported enough errors to repeat the previous frame: 6 for IMBE, 4 for AMBE"""
    rng = np.random.default_rng(seed)
    bits = (mbe.random_imbe_bits(rng, (S, F)) if codec == ddn.MBE_IMBE else mbe.random_ambe_bits(rng, (S, F)))
    res = np.zeros((S, F, 5), np.int32)
    res[..., 0] = 1
    res[..., 3] = 6 if codec == ddn.MBE_IMBE else 4
    res[..., 1] = 1
    res[..., 4] = res[..., 3] - res[..., 1]
    return bits, res


# ---- drivers: the restatement here, the device in the GPU file --------------------------------------------------------
class CpuDriver:
    def __init__(self, codec, S, first_stream=0):
        self.v = mbe.OracleVocoder(codec, S)
        self.codec, self.S, self.seed0 = codec, S, first_stream

    def set_state(self, s, cur, prev, enh):
        self.v.cur[s], self.v.prev[s], self.v.enh[s] = cur, prev, enh

    def state(self, s):
        return clone(self.v.cur[s]), clone(self.v.prev[s]), clone(self.v.enh[s])

    def run(self, bits, res_in=None):
        v = self.v
        bits = np.ascontiguousarray(bits, np.uint8)
        S, F = bits.shape[:2]
        pcm = np.zeros((S, F, 160), np.float32)
        res = np.zeros((S, F, 5), np.int32)
        ri = np.ascontiguousarray(res_in, np.int32) if res_in is not None else None
        rc = mbe._o().om_process_batch(self.codec, C.addressof(v.tab), bits.ctypes.data, ri.ctypes.data if ri is not None else None, 0,
                                       self.seed0, S, F, pcm.ctypes.data, res.ctypes.data, C.addressof(v.cur), C.addressof(v.prev),
                                       C.addressof(v.enh))
        assert rc == 0
        return pcm, res


# ---- the checks -----------------------------------------------------------------------------------------------------
class Figures(dict):
    """worst figures of a run, each as a fraction of its bound unless the name says otherwise"""

    def up(self, k, v):
        self[k] = max(self.get(k, 0.0), float(v))


def check_synth(fig, pcm, before_enh, after_enh, seed, frame_no, fails):
    ref, A = R.synth(R.Side.of(before_enh), R.Side.of(after_enh), seed, frame_no)
    d = np.abs(pcm.astype(np.float64) - ref)
    fig.up("synth |d|/bound", (d / (B_SYNTH * A + B_ABS)).max())
    if (A > 0).any():
        fig.up("synth |d|/A (absolute figure)", (d[A > 0] / A[A > 0]).max())
    if not np.all(d <= B_SYNTH * A + B_ABS):
        fails.append(("synth", int(np.argmax(d / (B_SYNTH * A + B_ABS)))))
    return ref, A


def check_enhance_phase(fig, unenh, before_enh, after_enh, seed, frame_no, fails, count):
    L = unenh.L
    want, cancel, _ = R.enhance(unenh.w0, L, unenh.Ml[:], details=True)
    got = np.array(after_enh.Ml[:], np.float32).astype(np.float64)
    live = np.arange(57)
    live = (live >= 1) & (live <= L)
    skip = live & (cancel < B_ENH)
    chk = live & ~skip
    count[0] += int(live.sum())
    count[1] += int(skip.sum())
    nz = chk & (want != 0.0)
    if nz.any():
        rel = np.abs(got[nz] - want[nz]) / want[nz]
        fig.up("enhance rel/bound", rel.max() / B_ENH)
        if rel.max() > B_ENH:
            fails.append(("enhance", float(rel.max())))
    if np.any(got[chk & (want == 0.0)] != 0.0):
        fails.append(("enhance zero", 0))
    e0 = float(np.sum(np.array(unenh.Ml[1:L + 1], np.float64) ** 2))
    e1 = float(np.sum(got[1:L + 1] ** 2))
    if e0 > 0.0:                                 # the restoring factor holds the energy whatever the weights were
        fig.up("energy rel/bound", abs(e1 - e0) / e0 / B_ENH)
        if abs(e1 - e0) > B_ENH * e0:
            fails.append(("energy", abs(e1 - e0) / e0))
    elif e0 == 0.0 and e1 != 0.0:
        fails.append(("energy zero", e1))
    num_uv = sum(1 for l in range(1, L + 1) if unenh.Vl[l] == 0)
    assert (before_enh.w0 + unenh.w0) * 56 * 80 <= 2900.0      # the premise of B_PHASE's derivation
    psi, phi = R.phases(R.Side.of(before_enh), R.Side.of(unenh), num_uv, seed, frame_no)
    gpsi, gphi = np.array(after_enh.PSIl[:], np.float32), np.array(after_enh.PHIl[:], np.float32)
    dpsi, dphi = R.circ(gpsi[1:], psi[1:]).max(), R.circ(gphi[1:], phi[1:]).max()
    fig.up("PSI circ/bound", dpsi / B_PHASE)
    fig.up("PHI circ/bound", dphi / B_PHASE)
    fig.up("|PSI| - pi (rad, absolute figure)", float(np.abs(gpsi[1:]).astype(np.float64).max()) - np.pi)
    if dpsi > B_PHASE or dphi > B_PHASE:
        fails.append(("phase", dpsi, dphi))
    if not np.all(np.abs(gpsi[1:]) <= PI32):
        fails.append(("PSI outside [-pi, pi]", float(np.abs(gpsi[1:]).max())))


def run_repeat_batch(make_driver, codec, cases, first_stream=0):
    """one repeat frame on every case -> (pcm [S][160], before [(cur, prev, enh)], after [...], seeds)"""
    S = len(cases)
    drv = make_driver(codec, S, first_stream)
    before = [case_triple(c) for c in cases]
    for s, t in enumerate(before):
        drv.set_state(s, *t)
    bits, res_in = repeat_frames(codec, S)
    pcm, res = drv.run(bits, res_in)
    assert np.all(res[..., 0] & REPEAT) and not np.any(res[..., 0] & MUTE)
    after = [drv.state(s) for s in range(S)]
    return pcm[:, 0], before, after, [first_stream + s for s in range(S)]


def check_repeat_synth(codec, cases, pcm, before, after, seeds):
    fig, fails = Figures(), []
    for s, c in enumerate(cases):
        f = []
        check_synth(fig, pcm[s], before[s][2], after[s][2], seeds[s], c["frame_no"], f)
        assert after[s][0].un == int(np.int32(np.uint32(c["frame_no"] + 1))) and after[s][0].repeat == 1
        fails += [(s, c["name"]) + x for x in f]
    print("codec %d synth: %s" % (codec, dict(fig)))
    assert not fails, fails
    return fig


def check_repeat_enhance_phase(codec, cases, before, after, seeds):
    fig, fails, count = Figures(), [], [0, 0]
    for s, c in enumerate(cases):
        f = []
        check_enhance_phase(fig, before[s][1], before[s][2], after[s][2], seeds[s], c["frame_no"], f, count)
        fails += [(s, c["name"]) + x for x in f]
    print("codec %d enhancement / phase: %s, %d of %d harmonics skipped" % (codec, dict(fig), count[1], count[0]))
    assert count[1] <= 0.01 * count[0], count
    assert not fails, fails
    return fig


def run_three_repeats(make_driver, codec=ddn.MBE_IMBE, f0=41):
    """three repeat frames as one call of three and as three calls of one, on a few of the cases; checks and returns the figures"""
    cases = build_cases()[::12]
    for c in cases:
        c["frame_no"] = f0
    S = len(cases)
    bits, res_in = repeat_frames(codec, S, 3)
    one = make_driver(codec, S, 0)
    three = make_driver(codec, S, 0)
    for s, c in enumerate(cases):
        one.set_state(s, *case_triple(c))
        three.set_state(s, *case_triple(c))
    pcm1, res1 = one.run(bits, res_in)
    fig, fails, count = Figures(), [], [0, 0]
    enh = [three.state(s)[2] for s in range(S)]
    for k in range(3):
        pcm, res = three.run(bits[:, k:k + 1], res_in[:, k:k + 1])
        assert np.all(res[..., 0] & REPEAT) and not np.any(res[..., 0] & MUTE) and np.array_equal(res[:, 0], res1[:, k])
        assert np.array_equal(pcm[:, 0].view(np.uint32), pcm1[:, k].view(np.uint32))
        for s in range(S):
            cur, prev, e = three.state(s)
            assert cur.un == f0 + k + 1 and cur.repeat == k + 1
            f = []
            # the hash is keyed with f0 + k, the previous side and the phase track continue from the state of frame k - 1
            check_synth(fig, pcm[s, 0], enh[s], e, s, f0 + k, f)
            check_enhance_phase(fig, prev, enh[s], e, s, f0 + k, f, count)
            fails += [(s, k) + x for x in f]
            enh[s] = e
    for s in range(S):
        assert all(mbe.parms_equal(a, b) for a, b in zip(one.state(s), three.state(s)))
    print("three repeats: %s" % dict(fig))
    assert not fails, fails
    return fig


def run_decoded_frames(make_driver, codec, S=8, F=6):
    rng = np.random.default_rng(31 + codec)
    bits = (mbe.random_imbe_bits if codec == ddn.MBE_IMBE else mbe.random_ambe_bits)(rng, (S, F))
    drv = make_driver(codec, S, 0)
    fig, fails, count = Figures(), [], [0, 0]
    enh = [drv.state(s)[2] for s in range(S)]
    for k in range(F):
        pcm, res = drv.run(bits[:, k:k + 1])
        assert not np.any(res[..., 0] & (REPEAT | MUTE))
        for s in range(S):
            cur, prev, e = drv.state(s)
            f = []
            check_synth(fig, pcm[s, 0], enh[s], e, s, k, f)
            check_enhance_phase(fig, prev, enh[s], e, s, k, f, count)
            L = prev.L
            lg = np.array(prev.log2Ml[1:L + 1], np.float32)
            assert 0.693 * np.abs(lg).max() < 16.0              # the premise of B_ML's derivation: the product rounds at 2^-21
            want = R.ml_from_log2(lg, np.array(prev.Vl[1:L + 1]), prev.w0, codec)
            rel = np.abs(np.array(prev.Ml[1:L + 1], np.float32).astype(np.float64) - want) / want
            fig.up("Ml rel/bound", rel.max() / B_ML)
            if rel.max() > B_ML:
                f.append(("Ml", float(rel.max())))
            fails += [(s, k) + x for x in f]
            enh[s] = e
    print("codec %d decoded frames: %s, %d of %d harmonics skipped" % (codec, dict(fig), count[1], count[0]))
    assert count[1] <= 0.01 * count[0], count
    assert not fails, fails
    return fig


# ---- the tests (CPU: the restatement) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return build_cases()


@pytest.fixture(scope="module")
def cpu_runs(cases):
    return {codec: run_repeat_batch(CpuDriver, codec, cases) for codec in CODECS}


def test_cases_cover_what_they_claim(cases):
    """every L of the list on either side, L above / below / equal, every voicing pair on one harmonic, harmonics on both sides of
    UVTHRESHOLD, every frame number"""
    assert len(cases) == 96
    for L in (9, 10, 12, 13, 36, 37, 55, 56):
        assert any(c["prev"][1] == L for c in cases) and any(c["cur"][1] == L for c in cases)
    rel = {np.sign(c["cur"][1] - c["prev"][1]) for c in cases}
    assert rel == {-1, 0, 1}
    seen = set()
    for c in cases:
        m = min(c["cur"][1], c["prev"][1])
        seen |= {(int(a), int(b)) for a, b in zip(c["prev"][2][1:m + 1], c["cur"][2][1:m + 1])}
        for side in ("prev", "cur"):
            w0l = np.float32(c[side][0]) * np.arange(1, c[side][1] + 1, dtype=np.float32)
            uv = c[side][2][1:c[side][1] + 1] == 0
            seen |= {"above"} if np.any(uv & (w0l > R.UVTHRESHOLD)) else set()
    assert seen >= {(0, 0), (0, 1), (1, 0), (1, 1), "above"}
    assert {c["frame_no"] for c in cases} >= {0, 1, 2 ** 31 - 1}


@pytest.mark.parametrize("codec", CODECS)
def test_synth_against_float64(cpu_runs, cases, codec):
    """|pcm[n] - ref[n]| <= 2^-14 A[n] + 2^-20 on all 160 samples of every case, seeds 0..95 and a non-zero first stream.
    Measured (restatement; both codecs run the same states): worst |d| / A = 1.29e-5, 0.21 of the bound; 9.1e-6 behind the
    non-zero first stream."""
    fig = check_repeat_synth(codec, cases, *cpu_runs[codec])
    few = cases[:8]
    check_repeat_synth(codec, few, *run_repeat_batch(CpuDriver, codec, few, FIRST_STREAM))
    assert fig["synth |d|/A (absolute figure)"] > 2.0 ** -26     # the comparison is not vacuous: binary32 rounding is seen


@pytest.mark.parametrize("codec", CODECS)
def test_enhancement_and_phase_against_float64(cpu_runs, cases, codec):
    """enhanced amplitudes within 2^-18 relative of enhance() (harmonics whose x is an ill-conditioned 0 / 0 skipped, at most 1 %),
    energy kept within 2^-18, PSIl / PHIl within 2^-11 rad circularly, PSIl in [-pi, pi].

    2^-11 rad: the unwrapped track reaches (pw0 + cw0) * 56 * 80 <= 2900 rad (asserted).  Rounding pw0 + cw0 at 2^-24 relative
    carries to 2900 * 2^-24 = 1.7e-4; the product and the sum with the previous PSIl each round at half an ulp of [2048, 4096)
    = 1.2e-4; the wrap subtracts k <= 462 times a binary32 2 pi that is 1.75e-7 too large = 0.8e-4; the fused wrap itself
    rounds below pi at 1.2e-7.  Sum 4.9e-4 = 2^-11.
    Measured (restatement): enhancement 0.084 of its bound, energy 0.11, PSIl 0.73, PHIl 0.73; none of 2969 harmonics skipped,
    |PSIl| never above the binary32 pi."""
    pcm, before, after, seeds = cpu_runs[codec]
    check_repeat_enhance_phase(codec, cases, before, after, seeds)


def test_three_repeats_keep_phase_and_counter():
    """three repeat frames in one call == three calls of one frame bit for bit; the counter, the repeat count, the phase track and
    the hash's frame number continue frame to frame.  Measured: synthesis 0.13 of its bound, enhancement 0.07, PSIl 0.58."""
    run_three_repeats(CpuDriver)


@pytest.mark.parametrize("codec", CODECS)
def test_decoded_frames_against_float64(codec):
    """8 paths x 6 ordinary random frames, one per call: synthesis, enhancement, phases as above and Ml within 2^-20 relative of
    exp(0.693 log2Ml) (times 0.2046 / sqrt(w0) on unvoiced AMBE bands).  2^-20: 0.693f * x rounds at half an ulp of [8, 16) = 2^-21
    while |0.693 x| < 16 (asserted; frames of the placeholder tables reach |x| = 16.8), the
    polynomial adds 8.3e-8 and the AMBE factor three roundings at 2^-24: 7.4e-7 < 2^-20 = 9.5e-7.
    Measured (IMBE / AMBE): Ml 0.49 / 0.34 of the bound, synthesis 0.26 / 0.10 (|d| / A = 1.56e-5 / 6.2e-6), enhancement 0.98 /
    0.08 - the 0.98 is harmonic 13 of a 30-harmonic spectrum that spans six decades, where num cancels to 1.8 % of its terms and
    the binary32 sums' error is amplified 55 x; it is the worst of 1740 harmonics, the next is at 0.35."""
    run_decoded_frames(CpuDriver, codec)


# ---- mutation checks --------------------------------------------------------------------------------------------------
def test_mutations_exceed_the_bounds(cpu_runs, cases):
    """each of five single mistakes (listed in the measured line), made in the model on the same inputs, misses its bound by at least 100 x - so the
    bounds can fail.  Measured: window + 1 sample 2.4e5 x, n for n - 160 2.8e4 x, -PHI 3.0e4 x, clamp 1.25 1.1e4 x, l * 160 6.4e3 x"""
    pcm, before, after, seeds = cpu_runs[ddn.MBE_IMBE]
    worst = {"window": 0.0, "origin": 0.0, "phi": 0.0, "clamp": 0.0, "step": 0.0}
    for s, c in enumerate(cases):
        p, e = R.Side.of(before[s][2]), R.Side.of(after[s][2])
        got = pcm[s].astype(np.float64)
        for key, kw in (("window", {"window_shift": 1}), ("origin", {"cur_origin": 0}), ("phi", {"phi_sign": -1.0})):
            ref, A = R.synth(p, e, seeds[s], c["frame_no"], **kw)
            worst[key] = max(worst[key], float((np.abs(got - ref) / (B_SYNTH * A + B_ABS)).max()))
        un = before[s][1]
        L = un.L
        want = R.enhance(un.w0, L, un.Ml[:], clamp_hi=1.25)[1:L + 1]
        g = np.array(after[s][2].Ml[1:L + 1], np.float64)
        nz = want != 0.0
        if nz.any():
            worst["clamp"] = max(worst["clamp"], float((np.abs(g[nz] - want[nz]) / want[nz]).max() / B_ENH))
        nuv = sum(1 for l in range(1, L + 1) if un.Vl[l] == 0)
        psi, _ = R.phases(R.Side.of(before[s][2]), R.Side.of(un), nuv, seeds[s], c["frame_no"], half=160)
        worst["step"] = max(worst["step"], float(R.circ(np.array(after[s][2].PSIl[1:]), psi[1:]).max() / B_PHASE))
    print("mutations, worst miss as a multiple of the bound:", worst)
    assert all(v >= 100.0 for v in worst.values()), worst


# ---- the elementary functions, compiled for the host ----------------------------------------------------------------
SRC = r'''
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#define __host__
#define __device__
#define __forceinline__ inline
#include "ddn_mbe_math.h"
#include "ddn_oracle_mbe_math.h"
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
int main() {
    const double ranges[3] = {8.0, 512.0, 4096.0};
    const int P = 4000000;
    double cos_err = 0.0, exp_err = 0.0;
    unsigned long long diff = 0;
    for (int r = 0; r < 3; r++) {
        for (int i = 0; i <= P; i++) {
            const float x = (float)(ranges[r] * (2.0 * (double)i / (double)P - 1.0));
            const float c = mbe_cosf(x);
            const double e = fabs((double)c - cos((double)x));
            cos_err = e > cos_err ? e : cos_err;
            diff += bits(c) != bits(om_cosf(x));
        }
    }
    for (int i = 0; i <= P; i++) {
        const float y = (float)(40.0 * (2.0 * (double)i / (double)P - 1.0));
        const float v = mbe_expf(y);
        const double t = exp((double)y), e = fabs((double)v - t) / t;
        exp_err = e > exp_err ? e : exp_err;
        diff += bits(v) != bits(om_expf(y));
    }
    const float edge[6] = {86.9f, 87.0f, 87.5f, -86.9f, -87.0f, -200.0f};
    for (int i = 0; i < 6; i++) {
        diff += bits(mbe_expf(edge[i])) != bits(om_expf(edge[i]));
    }
    uint32_t h = 1u;
    for (int i = 0; i < P; i++) {
        const uint32_t a = mbe_mix(h, (uint32_t)i), b = om_mix(h, (uint32_t)i);
        diff += a != b;
        diff += bits(mbe_u01(a)) != bits(om_u01(b));
        diff += bits(mbe_rand_phase(a)) != bits(om_rand_phase(b));
        h = a;
    }
    for (int k = -400; k <= 800; k++) {
        diff += bits(mbe_ws(k)) != bits(om_ws(k));
    }
    printf("%.6e %.6e %llu\n", cos_err, exp_err, diff);
    return 0;
}
'''


def test_elementary_functions_against_libm_and_each_other():
    """dsd-neo_amd/csrc/ddn_mbe_math.h compiled for the host: mbe_cosf against double cos on 4e6 points in each of |x| <= 8, 512,
    4096 (the kernels' arguments stay below 512), absolute; mbe_expf against double exp on |y| <= 40, relative; both <= 2^-22.
    Measured here: 9.5e-8 absolute, 8.3e-8 relative.  Over the same sweeps om_cosf, om_expf, om_mix, om_u01, om_rand_phase and
    om_ws of oracle/ddn_oracle_mbe_math.h equal the product's functions bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-I", os.path.join(root, "dsd-neo_amd", "csrc"),
                               "-I", os.path.join(root, "oracle"), os.path.join(d, "t.cpp"), "-o", exe, "-lm"])
        cos_err, exp_err, diff = subprocess.check_output([exe]).split()
    print("mbe_cosf abs %s, mbe_expf rel %s, differing results %s" % (cos_err.decode(), exp_err.decode(), diff.decode()))
    assert float(cos_err) <= 2.0 ** -22 and float(exp_err) <= 2.0 ** -22 and int(diff) == 0


# ---- the generator that replaced rand() -----------------------------------------------------------------------------
def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float(np.sum(a * b) / np.sqrt(np.sum(a * a) * np.sum(b * b)))


def test_generator_statistics():
    """mbe_u01 over 2^16 consecutive keys, in the order the synthesis draws them (harmonic l, sub-oscillator i, sample n): mean
    within 4 sigma of 1/2 (sigma = 1 / sqrt(12 N)); the three sub-oscillator phases of a harmonic pairwise uncorrelated (|r| < 4 /
    sqrt(N), 2^16 harmonics' keys); the noise of adjacent samples uncorrelated (|r| < 4 / sqrt(N)).
    Measured: mean - 1/2 = -0.72 sigma; adjacent samples 0.09 of the bound; phases 0.13, 0.32, 0.15 of the bound."""
    Nk = 1 << 16
    fbase = R.frame_key(3, 17)
    k = np.arange(Nk)
    l, i, n = k // 480 + 1, (k // 160) % 3, k % 160
    base = R.mix(fbase, l.astype(np.uint64))
    u = R.u01(R.mix(R.mix(base, (0x200 + 0x40 + i).astype(np.uint64)), n.astype(np.uint64)))
    sigma = 1.0 / np.sqrt(12.0 * Nk)
    print("mean - 1/2 = %.3f sigma" % ((u.mean() - 0.5) / sigma))
    assert abs(u.mean() - 0.5) <= 4.0 * sigma
    same = (l[1:] == l[:-1]) & (i[1:] == i[:-1])
    r_adj = _corr(u[:-1][same], u[1:][same])
    print("adjacent-sample correlation %.3f of 4 / sqrt(N)" % (r_adj * np.sqrt(same.sum()) / 4.0))
    assert abs(r_adj) < 4.0 / np.sqrt(same.sum())
    hb = R.mix(fbase, np.arange(1, Nk + 1, dtype=np.uint64))
    ph = [R.rand_phase(R.mix(hb, 0x200 + j)) for j in range(3)]
    for a, b in ((0, 1), (1, 2), (0, 2)):
        r = _corr(ph[a], ph[b])
        print("phase correlation (%d, %d) %.3f of 4 / sqrt(N)" % (a, b, r * np.sqrt(Nk) / 4.0))
        assert abs(r) < 4.0 / np.sqrt(Nk)
        assert abs(ph[a].mean()) <= 4.0 * 2.0 * np.pi * sigma
