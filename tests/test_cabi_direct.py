"""CPU: the entry points of the C ABI that need no device, called by name (tests/test_cabi_called.py keeps every exported function
reached by a test): the version strings, mbelib's float-to-short conversion, and the vocoder rates that are present but not
restated, which must say so and write silence."""
import ctypes as C

import numpy as np

import ddn

UNSUPPORTED, MUTE = -4, 0x10


def test_version_strings(built):
    l = ddn.lib()
    assert l.ddn_version().startswith(b"dsdneo-hip")
    assert b"mbelib-neo 2.0" in l.mbe_versionString()


def test_float_to_short_is_mbelibs(built):
    """gain 7, clipped to +-32760, truncated toward zero; null pointers are ignored"""
    l = ddn.lib()
    f = np.array([0.0, 1.0, -1.0, 0.99, -0.5, 5000.0, -5000.0, 4680.1, 4679.9, -4680.1, 1.0 / 7.0, -1.0 / 7.0] + [0.25] * 148, np.float32)
    sh = np.full(160, 77, np.int16)
    l.mbe_floattoshort(f.ctypes.data, sh.ctypes.data)
    want = np.trunc(np.clip(np.float32(7.0) * f, np.float32(-32760.0), np.float32(32760.0))).astype(np.int16)
    assert np.array_equal(sh, want) and sh[:8].tolist() == [0, 7, -7, 6, -3, 32760, -32760, 32760]
    l.mbe_floattoshort(None, sh.ctypes.data)
    l.mbe_floattoshort(f.ctypes.data, None)
    assert np.array_equal(sh, want)


def test_rates_that_are_not_restated_say_so(built):
    l = ddn.lib()
    res = ddn.MbeProcessResult(0xFF, 3, 3, 3, 3)
    fr, d = np.ones((7, 24), np.uint8), np.ones(88, np.uint8)
    assert l.mbe_decodeImbe7100x4400Frame(fr.ctypes.data, d.ctypes.data, C.byref(res)) == UNSUPPORTED
    assert not d.any() and bytes(res) == bytes(ddn.MbeProcessResult(MUTE, 0, 0, 0, 0))
    assert l.mbe_decodeImbe7100x4400Frame(None, d.ctypes.data, None) == -1 and l.mbe_decodeImbe7100x4400Frame(fr.ctypes.data, None, None) == -1
    assert l.mbe_decodeImbe7100x4400Frame(fr.ctypes.data, d.ctypes.data, None) == UNSUPPORTED

    pcm, ad = np.ones(160, np.float32), np.zeros(49, np.uint8)
    res = ddn.MbeProcessResult(0xFF, 3, 3, 3, 3)
    assert l.mbe_processAmbe2400Dataf(pcm.ctypes.data, C.byref(res), ad.ctypes.data, None, None, None) == UNSUPPORTED
    assert not pcm.any() and bytes(res) == bytes(ddn.MbeProcessResult(MUTE, 0, 0, 0, 0))
    pcm[:] = 1.0
    assert l.mbe_processAmbe2400Dataf(None, None, ad.ctypes.data, None, None, None) == -1
    assert l.mbe_processAmbe2400Dataf(pcm.ctypes.data, None, None, None, None, None) == -1 and pcm.all()

    fr4, d49 = np.ones((4, 24), np.uint8), np.ones(49, np.uint8)
    res = ddn.MbeProcessResult(0xFF, 3, 3, 3, 3)
    assert l.mbe_processAmbe3600x2400Framef(pcm.ctypes.data, C.byref(res), fr4.ctypes.data, d49.ctypes.data, None, None, None) == UNSUPPORTED
    assert not pcm.any() and not d49.any() and bytes(res) == bytes(ddn.MbeProcessResult(MUTE, 0, 0, 0, 0))
    for args in ((None, fr4.ctypes.data, d49.ctypes.data), (pcm.ctypes.data, None, d49.ctypes.data), (pcm.ctypes.data, fr4.ctypes.data, None)):
        assert l.mbe_processAmbe3600x2400Framef(args[0], None, args[1], args[2], None, None, None) == -1
