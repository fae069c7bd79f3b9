"""CPU: the dPMR superframe / chain entries (include/ddn_fsk4.h, include/ddn_chain.h) are exported and declared, the ctypes mirror of
ddn_dpmr_chain_results matches the C layout, the air-interface ID helper writes what the reference's dpmr_convert_air_interface_id()
writes, the generated colour-code table is the golden one, and the test encoder (tests/dpmrgen.py) round-trips through the restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import ddn
import dpmr
import dpmrgen

NAMES = ("ddn_dpmr_superframe_decode_batch", "ddn_dpmr_identity_batch", "ddn_dpmr_voice_gather", "ddn_dpmr_air_interface_id",
         "ddn_fsk4_chain_get_dpmr_results")


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_fsk4.h")).read() + open(os.path.join(ddn.ROOT, "include", "ddn_chain.h")).read()
    l = C.CDLL(ddn.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hdr, name
        assert hasattr(l, name), name
        assert name in ddn.PROTOTYPES, name


def test_ctypes_mirror_matches_the_header(built, tmp_path):
    fields = [f[0] for f in ddn.DpmrChainResults._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ddn_chain.h\"\nint main(void) {\n"
                   "    printf(\"%zu\\n\", sizeof(ddn_dpmr_chain_results));\n"
                   + "".join("    printf(\"%%zu\\n\", offsetof(ddn_dpmr_chain_results, %s));\n" % f for f in fields)
                   + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ddn.ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(ddn.DpmrChainResults)] + [getattr(ddn.DpmrChainResults, f).offset for f in fields]
    assert got == want, (fields, got, want)


def test_get_dpmr_results_refuses_a_null_chain(built):
    assert ddn.lib().ddn_fsk4_chain_get_dpmr_results(None, C.byref(ddn.DpmrChainResults())) == -1


def test_air_interface_id_equals_the_restatement_and_the_reference_rule(built):
    for val, s in dpmr.vectors()["aiid"]:
        assert ddn.dpmr_air_interface_id(val) == s == dpmr.air_interface_id(val)
    rng = np.random.default_rng(5)
    for v in list(rng.integers(0, 11 * 1464100, 2000)) + [0, 10, 1464099, 1464100 * 10, 11 * 1464100 - 1]:
        assert ddn.dpmr_air_interface_id(v) == dpmr.air_interface_id(int(v)), v
    # at and above 11 x 1464100 the reference writes the first digit as '0' + 11 (the restatement's "11" is not the reference's rule)
    for v in [11 * 1464100, 11 * 1464100 + 1, (1 << 24) - 1] + list(rng.integers(11 * 1464100, 1 << 24, 200)):
        v = int(v)
        want = ";" + dpmr.air_interface_id(v % 1464100).rjust(7, "0")[1:]
        assert ddn.dpmr_air_interface_id(v) == want, v
    assert ddn.dpmr_air_interface_id(11 * 1464100) == ";000000"


def test_generated_colour_table_is_the_golden_one():
    txt = open(os.path.join(ddn.ROOT, "dsd-neo_amd", "csrc", "ddn_tables_dpmr.h")).read()
    m = re.search(r"ddn_dpmr_color_codes\[64\]\[2\] = \{(.*?)\};", txt, re.S)
    rows = [[int(a, 16), int(b)] for a, b in re.findall(r"\{0x([0-9a-f]+)u, (\d+)u\}", m.group(1))]
    assert rows == dpmr.vectors()["color_codes"]


def test_encoder_round_trips_through_the_restatement():
    rng = np.random.default_rng(11)
    for _ in range(40):
        kw = dict(fn=int(rng.integers(0, 4)), half=int(rng.integers(0, 4096)), mode=int(rng.integers(0, 8)), version=int(rng.integers(0, 4)),
                  format=int(rng.integers(0, 4)), emergency=int(rng.integers(0, 2)), reserved=int(rng.integers(0, 2)),
                  slow=int(rng.integers(0, 1 << 18)))
        bits = dpmrgen.cch_bits(**kw)
        flips = [(j, int(rng.integers(0, 12))) for j in range(6) if rng.random() < 0.5]      # one error per word at most: corrected
        got = dpmr.decode_cch(dpmrgen.cch_dibits(bits, flips))
        assert got["ham_ok"] and got["crc_ok"] and list(got["bits48"]) == bits
        assert (got["fn"], got["mode"], got["version"], got["format"], got["emergency"], got["reserved"], got["slow"]) == (
            kw["fn"], kw["mode"], kw["version"], kw["format"], kw["emergency"], kw["reserved"], kw["slow"])
        bad = dpmr.decode_cch(dpmrgen.cch_dibits(dpmrgen.cch_bits(**kw, crc_good=False)))
        assert bad["ham_ok"] and not bad["crc_ok"]
    for col in (0, 17, 63):
        sf = dpmrgen.superframe(dpmrgen.cch_dibits(dpmrgen.cch_bits()), dpmrgen.cch_dibits(dpmrgen.cch_bits(fn=1)), dpmrgen.color_pattern(col),
                                [[0] * 36] * 8)
        assert dpmr.superframe(sf)["color"] == col
        assert dpmr.superframe(sf ^ 2, inverted=1)["color"] == col
