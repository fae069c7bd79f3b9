"""CPU: the DMR MS / direct-mode entries (include/ddn_fsk4.h, include/ddn_chain.h) are exported and declared, the ctypes mirrors of their
structs match the C layout a compiled probe reports, and every entry checks its arguments before it touches a device."""
import ctypes as C
import os
import subprocess

import ddn

NAMES = ("ddn_dmr_ms_state_bytes", "ddn_dmr_ms_state_init", "ddn_dmr_ms_walk_batch", "ddn_dmr_ms_data_batch", "ddn_dmr_ms_voice_batch",
         "ddn_fsk4_chain_set_dmr_ms", "ddn_fsk4_chain_get_dmr_ms_results")
STRUCTS = (("ddn_dmr_ms_input", "DmrMsInput"), ("ddn_dmr_ms_bursts", "DmrMsBursts"), ("ddn_dmr_ms_data", "DmrMsData"),
           ("ddn_dmr_ms_voice", "DmrMsVoice"), ("ddn_dmr_ms_chain_results", "DmrMsChainResults"))


def test_symbols_exported_and_declared(built):
    hdr = open(os.path.join(ddn.ROOT, "include", "ddn_fsk4.h")).read() + open(os.path.join(ddn.ROOT, "include", "ddn_chain.h")).read()
    l = C.CDLL(ddn.LIB_PATH)
    for name in NAMES:
        assert name + "(" in hdr, name
        assert hasattr(l, name), name
        assert name in ddn.PROTOTYPES, name
    assert "only serves the sync types without a restated handler" not in hdr


def test_ctypes_mirrors_match_the_header(built, tmp_path):
    lines, want = [], []
    for cname, pyname in STRUCTS:
        cls = getattr(ddn, pyname)
        fields = [f[0] for f in cls._fields_]
        lines.append("    printf(\"%%zu\\n\", sizeof(%s));\n" % cname)
        lines += ["    printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (cname, f) for f in fields]
        want += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    lines.append("    printf(\"%zu\\n\", offsetof(ddn_dmr_ms_chain_results, voice.d_pcm));\n")
    want.append(ddn.DmrMsChainResults.voice.offset + ddn.DmrMsVoice.d_pcm.offset)
    lines.append("    printf(\"%d\\n%d\\n%d\\n\", DDN_DMR_MS_LOCK_DATA, DDN_DMR_MS_LOCK_VOICE, DDN_DMR_MS_UNUSED == INT32_MIN);\n")
    want += [264, 1704, 1]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"ddn_chain.h\"\nint main(void) {\n" + "".join(lines) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ddn.ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want, (got, want)


def test_the_state_block_holds_the_fragment_store(built):
    """the open unit's position and next burst, the colour code, the dropped count and five 48-bit fragments of one bit per byte"""
    n = ddn.lib().ddn_dmr_ms_state_bytes()
    assert 4 * 4 + 5 * 48 <= n <= 320 and n % 4 == 0


def test_entries_check_their_arguments_before_the_device(built):
    l = ddn.lib()
    assert l.ddn_dmr_ms_state_init(None, 4, None) == ddn.DDN_EINVAL and b"ddn_dmr_ms_state_init" in l.ddn_last_error()
    assert l.ddn_dmr_ms_state_init(C.c_void_p(4096), 0, None) == ddn.DDN_EINVAL
    assert l.ddn_dmr_ms_walk_batch(None, None, None, None) == ddn.DDN_EINVAL and b"ddn_dmr_ms_walk_batch" in l.ddn_last_error()
    assert l.ddn_dmr_ms_data_batch(None, None, None, None) == ddn.DDN_EINVAL and b"ddn_dmr_ms_data_batch" in l.ddn_last_error()
    assert l.ddn_dmr_ms_voice_batch(None, None, None, None, None) == ddn.DDN_EINVAL and b"ddn_dmr_ms_voice_batch" in l.ddn_last_error()
    p = C.c_void_p(4096)                      # (never followed: every call below stops at its checks)
    full = dict(n_channels=2, max_symbols=1000, max_syncs=8, **{k: p for k, _ in ddn.DmrMsInput._fields_[3:]})

    def inp(**kw):
        v = dict(full)
        v.update(kw)
        return ddn.DmrMsInput(*[v[k] for k, _ in ddn.DmrMsInput._fields_])

    def bursts(hole=None, sizes=(3, 3, 2)):
        return ddn.DmrMsBursts(*sizes, *[None if k == hole else p for k, _ in ddn.DmrMsBursts._fields_[3:]])

    data, voice = ddn.DmrMsData(*[p] * 11), ddn.DmrMsVoice(*[p] * 8)
    for bad in (dict(n_channels=0), dict(max_syncs=0), dict(max_symbols=0), dict(d_records10=None), dict(d_counts=None), dict(d_new=None),
                dict(d_sync_pos=None), dict(d_sync_pat=None), dict(d_n_sync=None), dict(d_pre=None), dict(max_syncs=1 << 25)):
        assert l.ddn_dmr_ms_walk_batch(C.byref(inp(**bad)), p, C.byref(bursts()), None) == ddn.DDN_EINVAL, bad
    assert l.ddn_dmr_ms_walk_batch(C.byref(inp()), None, C.byref(bursts()), None) == ddn.DDN_EINVAL                         # no state
    for k, _ in ddn.DmrMsBursts._fields_[3:]:                                                                              # every list
        assert l.ddn_dmr_ms_walk_batch(C.byref(inp()), p, C.byref(bursts(hole=k)), None) == ddn.DDN_EINVAL, k
    for sizes in ((0, 3, 2), (3, 0, 2), (3, 3, 0), (3, -1, 2), ((1 << 20) + 1, 3, 2)):
        assert l.ddn_dmr_ms_walk_batch(C.byref(inp()), p, C.byref(bursts(sizes=sizes)), None) == ddn.DDN_EINVAL, sizes
        assert l.ddn_dmr_ms_data_batch(C.byref(inp()), C.byref(bursts(sizes=sizes)), C.byref(data), None) == ddn.DDN_EINVAL, sizes
        assert l.ddn_dmr_ms_voice_batch(C.byref(inp()), C.byref(bursts(sizes=sizes)), C.byref(voice), None, None) == ddn.DDN_EINVAL, sizes
    for bad in (dict(d_pre=None), dict(d_pre_rel=None), dict(d_records10=None)):
        assert l.ddn_dmr_ms_data_batch(C.byref(inp(**bad)), C.byref(bursts()), C.byref(data), None) == ddn.DDN_EINVAL, bad
    for k in ("d_data_start", "d_data_sync", "d_data_gate"):
        assert l.ddn_dmr_ms_data_batch(C.byref(inp()), C.byref(bursts(hole=k)), C.byref(data), None) == ddn.DDN_EINVAL, k
    for hole in range(11):
        d = ddn.DmrMsData(*[None if k == hole else p for k in range(11)])
        assert l.ddn_dmr_ms_data_batch(C.byref(inp()), C.byref(bursts()), C.byref(d), None) == ddn.DDN_EINVAL, hole
    for k in ("d_voice_start", "d_voice_pre", "d_voice_vc", "d_lc_pos", "d_lc_in128"):
        assert l.ddn_dmr_ms_voice_batch(C.byref(inp()), C.byref(bursts(hole=k)), C.byref(voice), None, None) == ddn.DDN_EINVAL, k
    for hole in range(5):
        v = ddn.DmrMsVoice(*[None if k == hole else p for k in range(8)])
        assert l.ddn_dmr_ms_voice_batch(C.byref(inp()), C.byref(bursts()), C.byref(v), None, None) == ddn.DDN_EINVAL, hole
    for hole in (5, 6, 7):                    # the vocoder's arrays are asked for only with a vocoder batch
        v = ddn.DmrMsVoice(*[None if k == hole else p for k in range(8)])
        assert l.ddn_dmr_ms_voice_batch(C.byref(inp()), C.byref(bursts()), C.byref(v), p, None) == ddn.DDN_EINVAL, hole
    assert l.ddn_fsk4_chain_set_dmr_ms(None, 1) == ddn.DDN_EINVAL and b"handlers = 1 and inverted = 0" in l.ddn_last_error()
    assert l.ddn_fsk4_chain_get_dmr_ms_results(None, C.byref(ddn.DmrMsChainResults())) == ddn.DDN_EINVAL
    assert b"ddn_fsk4_chain_set_dmr_ms" in l.ddn_last_error()
