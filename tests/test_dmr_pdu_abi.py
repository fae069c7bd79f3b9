"""CPU: the DMR data-PDU entries (include/ddn_fsk4.h, include/ddn_chain.h) are exported and declared, and the ctypes mirrors of
ddn_dmr_pdu_input, ddn_dmr_pdu_output and ddn_dmr_pdu_chain_results match the C layout a compiled probe reports."""
import ctypes as C
import os
import subprocess

import ddn

NAMES = ("ddn_dmr_pdu_state_bytes", "ddn_dmr_pdu_walk_batch", "ddn_dmr_pdu_marks_batch", "ddn_fsk4_chain_set_dmr_pdu_slots",
         "ddn_fsk4_chain_get_dmr_pdu_results")
STRUCTS = (("ddn_dmr_pdu_input", "DmrPduInput"), ("ddn_dmr_pdu_output", "DmrPduOutput"), ("ddn_dmr_pdu_chain_results", "DmrPduChainResults"))


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_fsk4.h")).read() + open(os.path.join(ddn.ROOT, "include", "ddn_chain.h")).read()
    l = C.CDLL(ddn.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hdr, name
        assert hasattr(l, name), name
        assert name in ddn.PROTOTYPES, name


def test_ctypes_mirrors_match_the_header(built, tmp_path):
    lines, want = [], []
    for cname, pyname in STRUCTS:
        cls = getattr(ddn, pyname)
        fields = [f[0] for f in cls._fields_]
        lines.append("    printf(\"%%zu\\n\", sizeof(%s));\n" % cname)
        lines += ["    printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (cname, f) for f in fields]
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    lines.append("    printf(\"%zu\\n\", offsetof(ddn_dmr_pdu_chain_results, out.d_pdu_header9));\n")
    want.append(ddn.DmrPduChainResults.out.offset + ddn.DmrPduOutput.d_pdu_header9.offset)
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ddn_chain.h\"\nint main(void) {\n" + "".join(lines) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ddn.ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, (got, want)


def test_the_state_block_holds_both_rows(built):
    """two 3072-byte dmr_pdu_sf rows, data_block_crc_valid and the scalars; a multiple of 4 (the rows are cleared by words)"""
    n = ddn.lib().ddn_dmr_pdu_state_bytes()
    assert 2 * 3072 + 2 * 127 < n < 2 * 3072 + 512 and n % 4 == 0


def test_entries_refuse_null_arguments(built):
    l = ddn.lib()
    assert l.ddn_fsk4_chain_get_dmr_pdu_results(None, C.byref(ddn.DmrPduChainResults())) == ddn.DDN_EINVAL
    assert l.ddn_fsk4_chain_set_dmr_pdu_slots(None, 4) == ddn.DDN_EINVAL and b"1 .. 8" in l.ddn_last_error()
    assert l.ddn_dmr_pdu_walk_batch(None, None, None, None) == ddn.DDN_EINVAL
    assert l.ddn_dmr_pdu_marks_batch(None, None, 0, None, 0, 0, None, None, None, 0, 0, None, None, None, None, None, 0, None) == ddn.DDN_EINVAL
    assert b"ddn_dmr_pdu_marks_batch" in l.ddn_last_error()
