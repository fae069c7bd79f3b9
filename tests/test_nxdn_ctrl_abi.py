"""CPU: the NXDN control-channel entries (include/ddn_fsk4.h, include/ddn_chain.h) are exported and declared, the ctypes mirrors of their
structs match the C layout a compiled probe reports, and every entry checks its arguments before it touches a device."""
import ctypes as C
import os
import subprocess

import ddn

NAMES = ("ddn_nxdn_ctrl_state_bytes", "ddn_nxdn_ctrl_state_init", "ddn_nxdn_ctrl_decode_batch", "ddn_nxdn_ctrl_walk_batch",
         "ddn_fsk4_chain_set_nxdn_ctrl", "ddn_fsk4_chain_get_nxdn_ctrl_results")
STRUCTS = (("ddn_nxdn_ctrl_input", "NxdnCtrlInput"), ("ddn_nxdn_ctrl_frames", "NxdnCtrlFrames"), ("ddn_nxdn_ctrl_messages", "NxdnCtrlMessages"),
           ("ddn_nxdn_ctrl_chain_results", "NxdnCtrlChainResults"))


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
    lines.append("    printf(\"%zu\\n\", offsetof(ddn_nxdn_ctrl_chain_results, messages.d_cac_fail));\n")
    want.append(ddn.NxdnCtrlChainResults.messages.offset + ddn.NxdnCtrlMessages.d_cac_fail.offset)
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ddn_chain.h\"\nint main(void) {\n" + "".join(lines) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ddn.ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, (got, want)


def test_the_state_block_holds_the_segment_store(built):
    """part_of_frame, last RAN, cac_fail, four CRC flags and four 18-bit segments of one bit per byte"""
    n = ddn.lib().ddn_nxdn_ctrl_state_bytes()
    assert 3 * 4 + 4 + 4 * 18 <= n <= 128 and n % 4 == 0


def test_entries_check_their_arguments_before_the_device(built):
    l = ddn.lib()
    assert l.ddn_nxdn_ctrl_state_init(None, 4, None) == ddn.DDN_EINVAL and b"ddn_nxdn_ctrl_state_init" in l.ddn_last_error()
    assert l.ddn_nxdn_ctrl_state_init(C.c_void_p(4096), 0, None) == ddn.DDN_EINVAL
    assert l.ddn_nxdn_ctrl_decode_batch(None, None, None) == ddn.DDN_EINVAL and b"ddn_nxdn_ctrl_decode_batch" in l.ddn_last_error()
    assert l.ddn_nxdn_ctrl_walk_batch(None, None, None, None, None) == ddn.DDN_EINVAL and b"ddn_nxdn_ctrl_walk_batch" in l.ddn_last_error()
    p = C.c_void_p(4096)                      # (never followed: every call below stops at its checks)
    full = dict(n_channels=2, max_symbols=1000, max_syncs=8, **{k: p for k, _ in ddn.NxdnCtrlInput._fields_[3:]})
    frames = ddn.NxdnCtrlFrames(*[p] * 7)
    msgs = ddn.NxdnCtrlMessages(*[p] * 7)

    def inp(**kw):
        v = dict(full)
        v.update(kw)
        return ddn.NxdnCtrlInput(*[v[k] for k, _ in ddn.NxdnCtrlInput._fields_])

    for bad in (dict(n_channels=0), dict(max_syncs=0), dict(max_symbols=0), dict(d_records10=None), dict(d_counts=None), dict(d_sync_pos=None),
                dict(d_n_sync=None), dict(max_syncs=1 << 25)):
        assert l.ddn_nxdn_ctrl_decode_batch(C.byref(inp(**bad)), C.byref(frames), None) == ddn.DDN_EINVAL, bad
    assert l.ddn_nxdn_ctrl_decode_batch(C.byref(inp()), C.byref(ddn.NxdnCtrlFrames(None, *[p] * 6)), None) == ddn.DDN_EINVAL     # d_kind
    assert b"d_kind" in l.ddn_last_error()
    for bad in (dict(n_channels=-1), dict(d_lich=None), dict(d_valid=None), dict(d_sacch=None), dict(d_sacch_ok=None), dict(d_sacch_hard=None),
                dict(d_sacch_hard_ok=None), dict(d_n_sync=None)):
        assert l.ddn_nxdn_ctrl_walk_batch(C.byref(inp(**bad)), C.byref(frames), p, C.byref(msgs), None) == ddn.DDN_EINVAL, bad
    assert l.ddn_nxdn_ctrl_walk_batch(C.byref(inp()), C.byref(frames), None, C.byref(msgs), None) == ddn.DDN_EINVAL                 # no state
    for hole in (0, 3, 5, 6):                 # d_kind, d_crc_ok, d_ran, d_sf feed the walk
        fr = ddn.NxdnCtrlFrames(*[None if k == hole else p for k in range(7)])
        assert l.ddn_nxdn_ctrl_walk_batch(C.byref(inp()), C.byref(fr), p, C.byref(msgs), None) == ddn.DDN_EINVAL, hole
    assert l.ddn_fsk4_chain_set_nxdn_ctrl(None, 1) == ddn.DDN_EINVAL and b"handlers = 1" in l.ddn_last_error()
    assert l.ddn_fsk4_chain_get_nxdn_ctrl_results(None, C.byref(ddn.NxdnCtrlChainResults())) == ddn.DDN_EINVAL
    assert b"ddn_fsk4_chain_set_nxdn_ctrl" in l.ddn_last_error()
