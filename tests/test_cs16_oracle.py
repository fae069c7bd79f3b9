"""What the cs16 GPU tests compare against, tied down on the CPU: the oracle's f32 entry on widened int16 equals the compiled
reference's f32 entry on the same floats, and the P25 control-channel capture still decodes to its known answer after the conversion
cu8 -> cs16 (a gain of 127.5 / 128, no offset) through the whole-stream CPU restatement."""
import numpy as np
import pytest

import chain_oracle
import cs16
import orc
from conftest import golden


def test_helpers():
    u = np.arange(256, dtype=np.uint8)
    s = cs16.cu8_to_cs16(u)
    assert s.dtype == np.int16 and s[0] == -32640 and s[255] == 32640 and np.all(np.diff(s.astype(np.int32)) == 256)
    # 256 (u - 127.5) / 32768 = (127.5 / 128) * (u - 127.5) / 127.5: the cu8 value at a fixed gain, exactly representable
    w = cs16.widen(s)
    assert w.dtype == np.float32 and np.array_equal(w.astype(np.float64), (u.astype(np.float64) - 127.5) / 128.0)
    e = cs16.widen(cs16.SALT)
    assert e[0, 0] == -1.0 and e[0, 1] == np.float32(32767.0 / 32768.0) and e[2, 0] == np.float32(-(2.0 ** -15)) and e[4, 0] == 0.0
    x = cs16.synth_c4fm_cs16(0, 3, 1000, 257, calls=[600, 400])
    for p in (7, 256 + 41, 257 - 3, 600 - 36, 1000 - 36):        # first tile, prefetched tile, block edge, the end of either call
        assert np.array_equal(x[0, p:p + 6], cs16.SALT), p
        assert np.array_equal(x[1, p + 1:p + 7], cs16.SALT), p


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (no reference tree at build time)")
@pytest.mark.parametrize("rate,profile,passes,squelch,blk", [(48000, 4, 0, 0.0, 2048), (24000, 1, 0, 0.0, 3000), (32000, 2, 0, 0.0, 257),
                                                             (48000, 4, 1, 0.0, 2048), (48000, 4, 0, 0.01, 2048)])
def test_oracle_f32_on_widened_cs16_equals_the_compiled_reference(built, rate, profile, passes, squelch, blk):
    n = 9000 - (9000 % (1 << passes))
    x = cs16.synth_c4fm_cs16(5, 1, n, blk)[0]
    if squelch:
        x[3000:6000] = 0
    w = np.ascontiguousarray(cs16.widen(x))
    want_o = orc.OracleFrontEnd(rate=rate, profile=profile, squelch=squelch, downsample_passes=passes).run_f32(w, blk)
    r = orc.ref()
    h = r.refh_fe_create(rate, 4800, 4, profile, 1, squelch, passes)
    out = np.zeros(n, np.float32)
    k = r.refh_fe_run_f32(h, w.ctypes.data, n, blk, out.ctypes.data)
    r.refh_fe_destroy(h)
    assert k == len(want_o) and cs16.same_bits(out[:k], want_o)


def test_control_channel_capture_as_cs16_still_reads_nac_140(built):
    """the known answer of the reference's full-chain test on this capture (NAC 0x140, tests/test_real_capture.py) after the
    conversion to cs16.  Asserted: every NID after the warm-up decodes clean (status 1, no corrected bit) to NAC 0x140 DUID 7, the
    frames lie 360 symbols apart, and every complete TSDU's first block passes its CRC - the same fields, with the same values, as
    the cu8 stream gives (the gain of 127.5 / 128 moves none of them)."""
    g = golden("iq_p25p1_c4fm_cc.npz")
    want_nac = int(bytes(g["expected_nac_hex"]).decode(), 16)
    assert want_nac == 0x140
    x = cs16.cu8_to_cs16(np.ascontiguousarray(g["iq"]))
    got = chain_oracle.run_channel(np.ascontiguousarray(cs16.widen(x)), 156, 2, 0, state={"fe": cs16.F32FrontEnd()})
    ref = chain_oracle.run_channel(np.ascontiguousarray(g["iq"]), 156, 2, 0)
    for r in (got, ref):
        nids = [n for n in r["nids"][1:] if n is not None]        # the first hit is a false sync before the threshold warm start
        assert len(nids) >= 24
        assert all(n[0] == 1 and n[1] == want_nac and n[2] == 7 and n[3] == 0 for n in nids)
        assert np.all(np.abs(np.diff(r["acc"][1:]) - 360) <= 1)
        assert len(r["tsbk_crc"]) >= 24 and sum(r["tsbk_crc"].values()) >= len(r["tsbk_crc"]) - 1
    assert len(got["acc"]) == len(ref["acc"]) and np.array_equal(got["acc"], ref["acc"])
    assert all(np.array_equal(got["tsbk"][i], ref["tsbk"][i]) for i in ref["tsbk"] if ref["tsbk_crc"][i])
