"""Edge streams for the CQPSK symbol-rate receive loop (oracle/ddn_oracle_cqrx.c, dsd-neo_amd/csrc/ddn_cqrx.hip): the inputs where
the slicer window's extrema, the extrema average and the soft-metric conversion can go wrong.  Each edge is written into a clean
carrier stream from `start` on, so a caller can put it where the loop is in frame (tests/test_oracle_cqrx.py drives the in-frame path
alone, tests/test_cqrx_fuzz_gpu.py the whole loop behind a sync).

Every loop symbol, hunting or in frame, writes slicer-window slot (symbol index mod 128), so index k lands in slot k % 128 on both
paths.  The window scan treats a NaN by where it sits: in slot 0 or 1 it seeds the extrema (and the result is NaN), further on every
compare with it is false and it is skipped.  Hence one NaN stream per case."""
import numpy as np

SSZ = 128
MAGNITUDES = (1e3, 1e6, 5e6, 1e7, 1.3e7, 1e9, 1e20, 3e38)  # (5e6 - 5e7: the soft metric passes 2^31)


def _at_slot(start, slot):
    """the first index >= start that lands in window slot `slot`"""
    return start + (slot - start) % SSZ


def _denormals(rng, n):
    tiny = np.float32(np.finfo(np.float32).tiny)
    v = (rng.random(n).astype(np.float32) * tiny).astype(np.float32)         # subnormals of both signs, the smallest among them
    v[::5] = np.float32(1.4e-45)
    v[1::7] = np.float32(-1.4e-45)
    return np.where(rng.random(n) < 0.5, v, -v).astype(np.float32)


def _exact_levels(rng, n):
    return np.array([1.0, 3.0, -1.0, -3.0], np.float32)[rng.integers(0, 4, n)]


def edge_names():
    return (["nan_slot0", "nan_slot1", "nan_later", "nan_run", "pinf", "ninf", "inf_both", "pzero_run", "nzero_run", "mixed_zero_run",
             "denormal_run", "constant", "exact_levels", "exact_thresholds"] + ["mag_%g" % m for m in MAGNITUDES])


def edge_stream(name, carrier, start, seed=0):
    """`carrier` (f32) with edge `name` written from index `start` on (start + 400 <= len(carrier))"""
    rng = np.random.default_rng(seed)
    s = np.array(carrier, np.float32, copy=True)
    n = len(s)
    assert start + 400 <= n, (start, n)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    if name == "nan_slot0":
        s[_at_slot(start, 0)] = nan
    elif name == "nan_slot1":
        s[_at_slot(start, 1)] = nan
    elif name == "nan_later":
        s[_at_slot(start, 77)] = nan
        s[_at_slot(start + 150, 5)] = -nan                                   # (sign bit set: a second NaN, elsewhere)
    elif name == "nan_run":
        k = _at_slot(start, 126)
        s[k:k + 5] = nan                                                     # slots 126, 127, 0, 1, 2
    elif name == "pinf":
        s[_at_slot(start, 3)] = inf
    elif name == "ninf":
        s[_at_slot(start, 0)] = -inf
    elif name == "inf_both":
        k = _at_slot(start, 40)
        s[k] = inf
        s[k + 1] = -inf
        s[k + 9] = inf
    elif name == "pzero_run":
        s[start:start + 140] = np.float32(0.0)
    elif name == "nzero_run":
        s[start:start + 140] = np.float32(-0.0)
    elif name == "mixed_zero_run":
        s[start:start + 200] = np.where(rng.random(200) < 0.5, np.float32(0.0), np.float32(-0.0))
    elif name == "denormal_run":
        s[start:start + 180] = _denormals(rng, 180)
        s[start + 40:start + 60] = np.float32(0.0)
    elif name == "constant":
        s[start:] = np.float32(1.0)
    elif name == "exact_levels":
        s[start:] = _exact_levels(rng, n - start)                           # no noise: the window is all ties
    elif name == "exact_thresholds":
        s[start:] = _exact_levels(rng, n - start)
        k = start + 150                                                      # the centre is exactly 0 by now: the slice thresholds
        s[k:k + 12] = [2.0, -2.0, 0.0, -0.0, 2.0, 2.0, -2.0, 0.0, 1.9999999, -2.0000002, 2.0000002, -1.9999999]
    elif name.startswith("mag_"):
        m = np.float32(float(name[4:]))
        k = _at_slot(start, 9)
        s[k] = m
        s[k + 200] = -m
        s[k + 201] = m                                                       # both signs in the window at once
    else:
        raise KeyError(name)
    return s
