"""GPU: the AMBE 3600x2450 single-frame drop-ins of include/ddn_mbe.h (mbelib-neo's names) - the siblings of the IMBE ones held in
tests/test_mbe_gpu.py.  They repack char[4][24] / mbe_soft_bit[4][24] into the batch layout and chain the frame decode into the
synthesis with the result flags carried between the two; everything here is bit for bit against the batch calls and the CPU
restatement.  Also ddn_mbe_batch_set_tables on a batch object."""
import ctypes as C

import numpy as np
import pytest

import ddn
import mbe
from test_mbe_gpu import GpuVocoder, gpu_frame_decode

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, INVALID_BITS = -1, -2
SOFT = 0x4


def _frames(seed=3, n=64):
    """n code words with 0..4 flipped bits each (beyond what the Golay words correct, so mis-corrections count too)"""
    rng = np.random.default_rng(seed)
    frames = np.stack([mbe.ambe_encode(d) for d in mbe.random_ambe_bits(rng, (n,))])
    for i in range(n):
        for pos in rng.choice(46, i % 5, replace=False):                   # distinct bits of rows 0 / 1, the two Golay words
            frames[i, pos // 23, pos % 23] ^= 1
    return frames, rng


def _fields(r):
    return [int(r.flags), r.c0_errors, r.c4_errors, r.total_errors, r.protected_errors]


def _soft(frames, rel):
    """-> mbe_soft_bit [n][4][24] as uint8 [n][4][24][2] {bit, reliability}"""
    return np.ascontiguousarray(np.stack([frames, rel], axis=-1).astype(np.uint8))


def test_ambe_decode_frame_hard(built):
    l = ddn.lib()
    frames, _ = _frames()
    want_bits, want_res, rc = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
    got_bits, got_res = gpu_frame_decode(ddn.MBE_AMBE, frames)
    assert (rc == 0).all() and len({int(t) for t in want_res[:, 3]}) >= 4          # clean and corrected words both
    for i in range(len(frames)):
        out = np.full(49, 9, np.uint8)
        r = ddn.MbeProcessResult(0xFFFF, 7, 7, 7, 7)
        assert l.mbe_decodeAmbe3600x2450Frame(frames[i].ctypes.data, out.ctypes.data, C.byref(r)) == 0
        assert np.array_equal(out, got_bits[i]) and np.array_equal(out, want_bits[i]), i
        assert _fields(r) == got_res[i].tolist() == want_res[i].tolist(), i
        assert r.flags & 1 and not r.flags & SOFT and r.protected_errors == r.total_errors - r.c0_errors
    out = np.full(49, 9, np.uint8)
    assert l.mbe_decodeAmbe3600x2450Frame(frames[7].ctypes.data, out.ctypes.data, None) == 0       # result == NULL is accepted
    assert np.array_equal(out, want_bits[7])
    bad = frames[7].copy()
    bad[2, 5] = 2
    r = ddn.MbeProcessResult(0xFFFF, 7, 7, 7, 7)
    assert l.mbe_decodeAmbe3600x2450Frame(bad.ctypes.data, out.ctypes.data, C.byref(r)) == INVALID_BITS
    assert l.mbe_decodeAmbe3600x2450Frame(None, out.ctypes.data, C.byref(r)) == INVALID_ARGUMENT
    assert l.mbe_decodeAmbe3600x2450Frame(bad.ctypes.data, None, C.byref(r)) == INVALID_ARGUMENT


def test_ambe_decode_frame_soft(built):
    l = ddn.lib()
    frames, rng = _frames(seed=4)
    want_bits, want_res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
    sure = np.full(frames.shape, 255, np.uint8)
    rel = rng.integers(0, 256, frames.shape, dtype=np.uint8)
    batch_bits, batch_res = gpu_frame_decode(ddn.MBE_AMBE, frames, rel)
    for i in range(len(frames)):
        out = np.full(49, 9, np.uint8)
        r = ddn.MbeProcessResult()
        assert l.mbe_decodeAmbe3600x2450SoftFrame(_soft(frames[i], sure[i]).ctypes.data, out.ctypes.data, C.byref(r)) == 0
        assert np.array_equal(out, want_bits[i]) and r.total_errors == want_res[i, 3] and r.c0_errors == want_res[i, 1], i
        assert r.flags & SOFT and r.flags & 1 and r.protected_errors == r.total_errors - r.c0_errors, i
        assert r.flags == want_res[i, 0] | SOFT, i
        out2 = np.full(49, 9, np.uint8)
        r2 = ddn.MbeProcessResult()
        assert l.mbe_decodeAmbe3600x2450SoftFrame(_soft(frames[i], rel[i]).ctypes.data, out2.ctypes.data, C.byref(r2)) == 0
        assert np.array_equal(out2, batch_bits[i]) and _fields(r2) == batch_res[i].tolist(), i
        assert r2.flags & SOFT
    bad = _soft(frames[0], sure[0])
    bad[1, 3, 0] = 2
    assert l.mbe_decodeAmbe3600x2450SoftFrame(bad.ctypes.data, np.zeros(49, np.uint8).ctypes.data, None) == INVALID_BITS
    assert l.mbe_decodeAmbe3600x2450SoftFrame(None, np.zeros(49, np.uint8).ctypes.data, None) == INVALID_ARGUMENT


def _triple():
    c, p, e = ddn.MbeParms(), ddn.MbeParms(), ddn.MbeParms()
    ddn.lib().mbe_initMbeParms(C.byref(c), C.byref(p), C.byref(e))
    return c, p, e


@pytest.mark.parametrize("soft", [False, True])
def test_ambe_process_frame_equals_decode_then_process(built, soft):
    """12 consecutive frames of one talk path: PCM, result and the {cur, prev, prev_enhanced} triple of the one-call entry point
    equal the two-call sequence's (decode, then mbe_processAmbe2450Dataf) and the CPU restatement's over the same frames"""
    l = ddn.lib()
    F = 12
    rng = np.random.default_rng(5 + soft)
    frames = np.stack([mbe.ambe_encode(d) for d in mbe.random_ambe_bits(rng, (F,))])
    frames[1, 0, 17] ^= 1
    frames[2, 1, 13:15] ^= 1
    for i in (4, 5, 6, 7, 8):                            # an error run, three corrected bits in each Golay word: repeats, then the mute
        frames[i, 0, 9 + i:12 + i] ^= 1             # (columns 12..23 hold the data bits, the ones that are counted)
        frames[i, 1, 12:15] ^= 1
    rel = rng.integers(0, 256, frames.shape, dtype=np.uint8)
    one, two = _triple(), _triple()
    if soft:
        bits, res = gpu_frame_decode(ddn.MBE_AMBE, frames, rel)
    else:
        bits, res, rc = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
        assert (rc == 0).all()
    o = mbe.OracleVocoder(ddn.MBE_AMBE, 1)
    want_pcm, want_res, rc = o.run(bits[None], res[None])
    assert rc == 0
    seen = 0
    for f in range(F):
        fr = _soft(frames[f], rel[f]) if soft else frames[f]
        dec = l.mbe_decodeAmbe3600x2450SoftFrame if soft else l.mbe_decodeAmbe3600x2450Frame
        fn = l.mbe_processAmbe3600x2450SoftFramef if soft else l.mbe_processAmbe3600x2450Framef
        d1, d2 = np.full(49, 9, np.uint8), np.full(49, 9, np.uint8)
        p1, p2 = np.full(160, 5.0, np.float32), np.full(160, 5.0, np.float32)
        r1, r2 = ddn.MbeProcessResult(0xFFFF, 7, 7, 7, 7), ddn.MbeProcessResult()
        assert fn(p1.ctypes.data, C.byref(r1), fr.ctypes.data, d1.ctypes.data, *[C.byref(t) for t in one]) == 0
        assert dec(fr.ctypes.data, d2.ctypes.data, C.byref(r2)) == 0
        assert l.mbe_processAmbe2450Dataf(p2.ctypes.data, C.byref(r2), d2.ctypes.data, *[C.byref(t) for t in two]) == 0
        assert np.array_equal(d1, d2) and np.array_equal(d1, bits[f]), f
        assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)) and _fields(r1) == _fields(r2), f
        assert all(mbe.parms_equal(a, b) for a, b in zip(one, two)), f
        assert np.array_equal(p1.view(np.uint32), want_pcm[0, f].view(np.uint32)) and _fields(r1) == want_res[0, f].tolist(), f
        assert bool(r1.flags & SOFT) == soft, f
        seen |= r1.flags
    assert all(mbe.parms_equal(a, b) for a, b in zip(one, (o.cur[0], o.prev[0], o.enh[0])))
    assert one[0].un > 0 and (soft or (seen & 0x8 and seen & 0x10))               # the hard run exercised repeat and mute


def test_ambe_process_frame_argument_rules(built):
    l = ddn.lib()
    frames, _ = _frames(seed=9, n=2)
    for soft in (False, True):
        fn = l.mbe_processAmbe3600x2450SoftFramef if soft else l.mbe_processAmbe3600x2450Framef
        fr = _soft(frames[0], np.full((4, 24), 255, np.uint8)) if soft else frames[0]
        c, p, e = _triple()
        d, pcm = np.zeros(49, np.uint8), np.full(160, 5.0, np.float32)
        r = ddn.MbeProcessResult()
        tri = [C.byref(c), C.byref(p), C.byref(e)]
        assert fn(None, C.byref(r), fr.ctypes.data, d.ctypes.data, *tri) == INVALID_ARGUMENT
        for args in ((None, d.ctypes.data, *tri), (fr.ctypes.data, None, *tri), (fr.ctypes.data, d.ctypes.data, None, tri[1], tri[2]),
                     (fr.ctypes.data, d.ctypes.data, tri[0], None, tri[2]), (fr.ctypes.data, d.ctypes.data, tri[0], tri[1], None)):
            pcm[:] = 5.0
            assert fn(pcm.ctypes.data, C.byref(r), *args) == INVALID_ARGUMENT and not pcm.any(), (soft, args)
        fresh = _triple()
        assert all(mbe.parms_equal(a, b) for a, b in zip((c, p, e), fresh))           # none of the refused calls moved the history
        bad = fr.copy()
        if soft:
            bad[0, 3, 0] = 2
        else:
            bad[0, 3] = 2
        pcm[:] = 5.0
        assert fn(pcm.ctypes.data, C.byref(r), bad.ctypes.data, d.ctypes.data, *tri) == INVALID_BITS and not pcm.any()
        assert all(mbe.parms_equal(a, b) for a, b in zip((c, p, e), fresh))
        # result == NULL works: the same PCM and history as with one
        c2, p2, e2 = _triple()
        pcm2, d2 = np.full(160, 5.0, np.float32), np.zeros(49, np.uint8)
        assert fn(pcm.ctypes.data, C.byref(r), fr.ctypes.data, d.ctypes.data, *tri) == 0
        assert fn(pcm2.ctypes.data, None, fr.ctypes.data, d2.ctypes.data, C.byref(c2), C.byref(p2), C.byref(e2)) == 0
        assert np.array_equal(pcm.view(np.uint32), pcm2.view(np.uint32)) and np.array_equal(d, d2)
        assert all(mbe.parms_equal(a, b) for a, b in zip((c, p, e), (c2, p2, e2)))


def test_init_process_result_zeroes_the_struct(built):
    l = ddn.lib()
    r = ddn.MbeProcessResult(0xFFFFFFFF, -1, 7, 1 << 30, -5)
    l.mbe_initProcessResult(C.byref(r))
    assert bytes(r) == bytes(C.sizeof(ddn.MbeProcessResult))
    l.mbe_initProcessResult(None)                        # a null pointer is ignored


def test_batch_table_blob_is_loadable(built):
    """ddn_mbe_batch_set_tables on a batch object (the drop-ins' own blob is tests/test_mbe_gpu.py::test_dropin_table_blob_is_loadable):
    a modified blob changes the batch's PCM to the restatement's PCM with that blob; a blob that fails validation is refused and
    the loaded one stays"""
    l = ddn.lib()
    rng = np.random.default_rng(17)
    t = mbe.tables()
    for i in range(64):
        t.imbe_gain_b2[i] *= 0.5
    for i in range(32):
        t.ambe_dg[i] += 0.25
    t.synthetic = 0
    S, F = 3, 5
    for codec, gen in ((ddn.MBE_IMBE, mbe.random_imbe_bits), (ddn.MBE_AMBE, mbe.random_ambe_bits)):
        bits = gen(rng, (S, F))
        dflt, _, _ = mbe.OracleVocoder(codec, S).run(bits)
        want, want_res, rc = mbe.OracleVocoder(codec, S, tab=t).run(bits)
        assert rc == 0 and not np.array_equal(want, dflt)
        g = GpuVocoder(codec, S)
        before, _ = g.run(bits)
        assert np.array_equal(before.view(np.uint32), dflt.view(np.uint32)) and l.ddn_mbe_batch_tables_synthetic(g.h) == 1
        g = GpuVocoder(codec, S)
        assert l.ddn_mbe_batch_set_tables(g.h, C.byref(t)) == 0 and l.ddn_mbe_batch_tables_synthetic(g.h) == 0
        bad = mbe.tables()
        bad.magic = 0
        assert l.ddn_mbe_batch_set_tables(g.h, C.byref(bad)) != 0 and l.ddn_mbe_batch_tables_synthetic(g.h) == 0
        assert l.ddn_mbe_batch_set_tables(g.h, None) != 0 and l.ddn_mbe_batch_set_tables(None, C.byref(t)) != 0
        after, res = g.run(bits)
        assert np.array_equal(after.view(np.uint32), want.view(np.uint32)) and np.array_equal(res, want_res), codec
