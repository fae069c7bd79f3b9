"""CPU, everywhere: the restatement of the audio-monitor kind against tests/golden/fm_audio_*.npz, what the compiled reference gave for
six configurations (tests/golden/make_golden_fm_audio.py), and the library's host-side design against both."""
import ctypes as C
import json

import numpy as np
import pytest

import ddn
import fm_audio
from fm_audio import bits


@pytest.mark.parametrize("name", sorted(fm_audio.GOLDEN))
def test_restatement_equals_golden(built, name):
    g = np.load(fm_audio.golden_path(name))
    c = json.loads(str(g["cfg_json"]))
    c["lpr"] = tuple(c["lpr"]) if c["lpr"] else None
    assert c == fm_audio.cfg(**fm_audio.GOLDEN[name])
    got, st = fm_audio.restate_batch(c, g["iq"], [int(m) for m in g["calls"]])
    assert got.shape == g["audio"].shape and np.array_equal(bits(got), bits(g["audio"]))
    assert np.array_equal(bits(st), bits(g["state"]))
    c3, t16 = fm_audio.Restatement(c).coefficients()
    assert np.array_equal(bits(t16), bits(g["taps"]))
    # the product's own design (host code, no device)
    ac = ddn.FmAudioConfig(post_downsample=c["M"], deemph=c["deemph"], deemph_tau_us=c["tau"], audio_lpf_cutoff_hz=c["lpf"])
    d3, d16 = np.zeros(3, np.float32), np.zeros(16, np.float32)
    assert ddn.lib().ddn_fm_audio_design(c["rate"], C.byref(ac), d3.ctypes.data, d16.ctypes.data) == 0
    assert np.array_equal(bits(d3), bits(c3)) and np.array_equal(bits(d16), bits(g["taps"]))


def test_fixtures_are_small():
    import os
    sizes = [os.path.getsize(fm_audio.golden_path(n)) for n in fm_audio.GOLDEN]
    assert sum(sizes) < 200 * 1024 and all(g["iq"].shape[:2] == (2, fm_audio.GOLDEN_N) for g in map(np.load, map(fm_audio.golden_path, fm_audio.GOLDEN)))
