"""CPU: the EDACS restatement (tests/edacs.py) against the reference's own vectors (tests/golden/edacs_vectors.json), the generator
(tests/edacsgen.py) through it under all four modes, the restated 9600_2 hunt (tests/edacs_rx.c) on the reference's capture (the known
answer "Site ID [02][002]"), and the C ABI of the new entries (exported, declared, ctypes layout, configuration refusals)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ddn
import edacs
import edacsgen
import rx4

NAMES = ("ddn_edacs_frame_decode_batch", "ddn_fsk4_chain_set_edacs_mode", "ddn_fsk4_chain_get_edacs_results")


def test_bch_equals_the_reference_vectors():
    v = edacs.vectors()
    for msg, cw in v["bch"]:
        assert edacs.bch(msg) == cw and (cw >> 12) == msg and cw < (1 << 40)
    a, b = v["bch_ignores_above_28"]
    assert a != b and edacs.bch(a) == edacs.bch(b)
    # linear and cyclic-systematic: the parity of a sum is the sum of the parities
    rng = np.random.default_rng(1)
    for _ in range(200):
        x, y = (int(t) for t in rng.integers(0, 1 << 28, 2))
        assert edacs.bch(x ^ y) == edacs.bch(x) ^ edacs.bch(y)


def test_sync_words_and_types():
    v = edacs.vectors()
    neg, pos = v["sync_words"]["EDACS_SYNC"], v["sync_words"]["INV_EDACS_SYNC"]
    assert len(neg["symbols"]) == len(pos["symbols"]) == 48
    assert all(a != b for a, b in zip(neg["symbols"], pos["symbols"]))
    # this project's type ids are the reference's + 1 (include/ddn_fsk4.h: DDN_EDACS_TYPE_NEG / _POS)
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_fsk4.h")).read()
    assert "#define DDN_EDACS_TYPE_NEG %d" % (neg["type"] + 1) in hdr and "#define DDN_EDACS_TYPE_POS %d" % (pos["type"] + 1) in hdr
    assert edacs.sync_word(edacs.PAT_NEG) == neg["symbols"] and edacs.sync_word(edacs.PAT_POS) == pos["symbols"]
    # the dotting words are no sync word and no one-symbol shift of one
    for d in v["dotting"].values():
        assert d not in (neg["symbols"], pos["symbols"])


def test_vote_and_frame_round_trip_every_mode():
    rng = np.random.default_rng(3)
    for mode, (ea, esk) in edacs.MODES.items():
        for k in range(60):
            m1 = edacsgen.ea_site_id_msg(int(rng.integers(0, 256)), int(rng.integers(0, 128)), esk) if ea else \
                edacsgen.site_id_msg(int(rng.integers(0, 32)), int(rng.integers(0, 8)), int(rng.integers(0, 32)), int(rng.integers(0, 2)),
                                     int(rng.integers(0, 2)), int(rng.integers(0, 2)), esk)
            m2 = int(rng.integers(0, 1 << 28))
            # one bad copy per bit position: the vote corrects it
            flips = [(3 * h + int(rng.integers(0, 3)), int(b)) for h in range(2) for b in rng.choice(40, 8, replace=False)]
            d = edacs.decode_bits(edacsgen.frame_bits(m1, m2, flips), ea, esk)
            assert d["frame_ok"] and d["bch_ok"] == [1, 1] and d["vote40"] == [edacs.bch(m1), edacs.bch(m2)], mode
            assert d["msg28"] == [m1 ^ (esk << 20), m2 ^ (esk << 20)] and d["kind"] == (4 if ea else 3), mode
            # two bad copies of one bit: the vote takes the wrong value, the re-encoding no longer matches
            h, b = k & 1, int(rng.integers(0, 40))
            bad = edacs.decode_bits(edacsgen.frame_bits(m1, m2, [(3 * h, b), (3 * h + 2, b)]), ea, esk)
            assert not bad["frame_ok"] and bad["bch_ok"][h] == 0 and bad["bch_ok"][1 - h] == 1 and bad["kind"] == 0, mode


def test_site_id_fields():
    m = edacsgen.site_id_msg(2, priority=5, cc_lcn=17, scat=1, failsoft=0, aux=1)
    kind, t, f = edacs.classify(m, 0, True)
    assert kind == 3 and t == [7, 7, 8] and f == [2, 5, 17, 1, 0, 1]
    assert edacs.site_line(f[0]) == "Site ID [02][002]"
    kind, t, f = edacs.classify(edacsgen.ea_site_id_msg(0xB7, 0x55), 1, True)
    assert kind == 4 and t == [0x1F, 0xA, 0] and f[:2] == [0xB7, 0x55]
    # the same message under the other ESK setting is some other message
    assert edacs.classify(m ^ (edacs.ESK << 20), 0, True)[0] != 3


@pytest.mark.parametrize("neg", [1, -1])
def test_restated_loop_reads_the_capture_site_id(neg):
    """DECODE_IQ_EDACS (tests/CMakeLists.txt:8958-8963) on the CPU: the capture as sent holds -EDACS words, I/Q swapped +EDACS words"""
    disc = rx4.capture_disc("iq_edacs.npz", 3)
    o = edacs.LoopRx(2).run(disc * neg)
    assert set(o["sync_pat"].tolist()) == {edacs.PAT_NEG if neg > 0 else edacs.PAT_POS}
    frames = edacs.decode_stream(o)
    assert len(frames) >= 60 and all(f["frame_ok"] for f in frames)
    assert {edacs.site_line(f["site6"][0]) for f in frames if f["kind"] == 3} == {"Site ID [02][002]"}


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_fsk4.h")).read() + open(os.path.join(ddn.ROOT, "include", "ddn_chain.h")).read()
    l = C.CDLL(ddn.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hdr, name
        assert hasattr(l, name), name
        assert name in ddn.PROTOTYPES, name
    assert ddn.FSK4_EDACS == 8 and "DDN_FSK4_EDACS = 8" in hdr


def test_ctypes_mirror_matches_the_header(built, tmp_path):
    fields = [f[0] for f in ddn.EdacsChainResults._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ddn_chain.h\"\nint main(void) {\n"
                   "    printf(\"%zu\\n\", sizeof(ddn_edacs_chain_results));\n"
                   + "".join("    printf(\"%%zu\\n\", offsetof(ddn_edacs_chain_results, %s));\n" % f for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ddn.ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(ddn.EdacsChainResults)] + [getattr(ddn.EdacsChainResults, f).offset for f in fields]
    assert got == want, (fields, got, want)


def test_configuration_refusals_without_a_device(built):
    """what the C entries refuse before they touch a device"""
    l = ddn.lib()
    for kw in (dict(handlers=1), dict(inverted=1), dict(vocoder=1), dict(rf_mod=1)):
        cfg = dict(rf_mod=2, inverted=0, handlers=0, vocoder=0)
        cfg.update(kw)
        c = ddn.Fsk4ChainConfig(2, 48000, 8192, 0, ddn.FSK4_EDACS, cfg["rf_mod"], cfg["inverted"], cfg["handlers"], cfg["vocoder"])
        h = C.c_void_p()
        assert l.ddn_fsk4_chain_create(C.byref(c), C.byref(h)) == -1 and not h.value, kw
    for rate, inv in ((48000, 1), (44100, 0), (24000, 0), (192000, 0)):
        rc = ddn.Fsk4RxConfig(2, rate, ddn.FSK4_EDACS, 2, inv, 1)
        h = C.c_void_p()
        assert l.ddn_fsk4_rx_create(C.byref(rc), C.byref(h)) < 0 and not h.value, (rate, inv)
    assert l.ddn_fsk4_chain_set_edacs_mode(None, 0, 0) == -1
    assert l.ddn_fsk4_chain_get_edacs_results(None, C.byref(ddn.EdacsChainResults())) == -1
    z = [None, 0, None, None, None, None, None]
    assert l.ddn_edacs_frame_decode_batch(*z, 1, 1, 0, 0x20, *([None] * 9), None) == -1          # esk_mask 0 or 0xA0 only
    assert l.ddn_edacs_frame_decode_batch(*z, 1, 1, 2, 0, *([None] * 9), None) == -1             # ea_mode 0 or 1
    assert l.ddn_edacs_frame_decode_batch(*z, 1, 1, 0, 0, *([None] * 9), None) == -1             # null pointers
    assert l.ddn_edacs_frame_decode_batch(*z, 0, 0, 1, 0xA0, *([None] * 9), None) == 0           # nothing to do
