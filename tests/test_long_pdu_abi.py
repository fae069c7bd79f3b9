"""CPU: the long data unit switch of the P25 chain (ddn_p25_chain_set_long_data_units / _get_long_pdu_results, include/ddn_chain.h)
is exported and declared, the ctypes mirror of its result struct matches the C layout, the calls refuse a NULL chain without touching
a device, and the test-side restatement (tests/long_pdu.py) recovers long units exactly on a CPU-only stream."""
import ctypes as C
import os
import subprocess

import numpy as np

import chain_stream
import ddn
import long_pdu
import p25gen

NAMES = ("ddn_p25_chain_set_long_data_units", "ddn_p25_chain_get_long_pdu_results")


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_chain.h")).read()
    l = C.CDLL(ddn.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hdr, name
        assert hasattr(l, name), name
        assert name in ddn.PROTOTYPES, name


def test_ctypes_mirror_matches_the_header(built, tmp_path):
    fields = [f[0] for f in ddn.P25LongPduResults._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ddn_chain.h\"\nint main(void) {\n"
                   "    printf(\"%zu\\n\", sizeof(ddn_p25_long_pdu_results));\n"
                   + "".join("    printf(\"%%zu\\n\", offsetof(ddn_p25_long_pdu_results, %s));\n" % f for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ddn.ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(ddn.P25LongPduResults)] + [getattr(ddn.P25LongPduResults, f).offset for f in fields]
    assert got == want, (fields, got, want)


def test_null_chain_is_refused(built):
    l = ddn.lib()
    r = ddn.P25LongPduResults()
    assert l.ddn_p25_chain_set_long_data_units(None, 127, 0) == ddn.DDN_EINVAL
    assert l.ddn_p25_chain_set_long_data_units(None, 0, 0) == ddn.DDN_EINVAL
    assert l.ddn_p25_chain_get_long_pdu_results(None, C.byref(r)) == ddn.DDN_EINVAL


def test_restatement_recovers_long_units_on_the_cpu(built):
    """9-, 40- and 127-block units (and a confirmed 12-block one) through the CPU stream restatement: the blocks are the data sent,
    every CRC32 holds; a short unit and a SAP 61 unit announcing 20 blocks (read as four) are not long"""
    rng = np.random.default_rng(5)
    nac = 0x293
    # (the loop leaves the SAP 61 unit after four blocks and hunts through its other sixteen: a TSDU lets it settle again)
    plan = [dict(blks=12, confirmed=True), dict(blks=9), dict(blks=3), dict(blks=40), dict(blks=127), dict(blks=20, sap=61), "tsdu"]
    parts = [p25gen.make_frames(rng, 1, nac, crc=True, blocks=1)[0], np.zeros(160, np.int8)]
    sent = []
    for kw in plan:
        if kw == "tsdu":
            parts += [p25gen.make_frames(rng, 1, nac, crc=True, blocks=1)[0], np.zeros(100, np.int8)]
            continue
        fr, hdr, data = p25gen.make_pdu_coded(rng, nac, **kw)
        sent.append((kw, hdr, data))
        parts += [fr, np.zeros(200, np.int8)]
    dib = np.concatenate(parts)
    n = len(dib) * 10 + 2000
    iq = p25gen.modulate_cu8(dib, n, lead=260, seed=3, noise=0.02)
    want = chain_stream.run_stream(iq, 48000, seed=0, vocoder=False)
    units = long_pdu.expected_units(want)
    long_sent = [s for s in sent if s[0]["blks"] > 8 and s[0].get("sap", 0) != 61]
    assert len(units) == len(long_sent), (sorted(units), [s[0] for s in long_sent])
    for (a, u), (kw, hdr, data) in zip(sorted(units.items()), long_sent):
        nb = kw["blks"]
        assert np.array_equal(u["header"], hdr), (kw, a)
        assert tuple(u["info"]) == (nb + 1, nb, 4 if kw.get("confirmed") else 0, 1), (kw, u["info"])
        assert u["valid"][:nb].all() and not u["valid"][nb:].any()
        if kw.get("confirmed"):
            assert np.array_equal(u["blocks18"][:nb], data) and u["crc9"][:nb].all()
        else:
            assert np.array_equal(u["blocks"][:nb], data)
