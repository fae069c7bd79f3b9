"""CPU: every function of the C ABI is reached by a test.  tests/test_cabi_exports.py proves that what include/*.h declares is
exported and bound; this file proves that it is also called.  For every name in ddn.PROTOTYPES one of these holds:

  1. the name occurs as a whole word in a tests/*.py file (other than test_cabi_exports.py, whose tables list names without
     exercising them, and this file) or in the body of a function of dsd-neo_amd/bindings/*.py - the wrappers the tests drive;
     the PROTOTYPES tables themselves stand at module level and do not count;
  2. it is a key of REACHED_THROUGH below: {name: the tested entry point that calls it}.  The caller must itself satisfy rule 1 and
     the callee's name must occur in the source file that defines the caller.  Each entry was checked by reading the caller.

A new export without a test fails here until it gets one."""
import ast
import os
import re

import ddn

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ddn.ROOT, "dsd-neo_amd", "csrc")
BINDINGS = os.path.join(ddn.ROOT, "dsd-neo_amd", "bindings")

# the host-buffer variant stages its buffers and calls the device-pointer variant of the same name
_HOST = ("ddn_fec_viterbi_k5", "ddn_fec_p25_lsd", "ddn_fec_rs28", "ddn_audio_s16", "ddn_fec_isch_lookup", "ddn_fec_golay24_soft",
         "ddn_fec_hamming_10_6_3_soft", "ddn_fec_p25_rs_soft", "ddn_fec_p25_12_soft_list", "ddn_fec_rs_12_9", "ddn_audio_agf",
         "ddn_p25p2_ess", "ddn_p25p2_burst_fields")
REACHED_THROUGH = {name + "_batch": name + "_host" for name in _HOST}
REACHED_THROUGH.update({
    "ddn_fsk4_rx_set_events": "ddn_fsk4_rx_events_host_arm",          # arms the object's own buffers through the setter
    "ddn_fec_bptc_128x77_batch": "ddn_fsk4_chain_run",                # the DMR section's embedded-signalling stage
    "ddn_p25_rx_set_event_data": "ddn_p25_chain_run",                 # the chain's loop stage points the loop at its payload rows
    "ddn_p25p1_framer_device_dropped": "ddn_p25_chain_get_results",
    "ddn_p25p1_framer_device_syncs": "ddn_p25_chain_get_results",
    "ddn_p25_chain_set_first_channel": "ddn_node_create",             # every part's talk paths are numbered by its first channel
    "ddn_iq_effective_bytes": "ddn_iq_capture_open",
})


def _source(path):
    with open(path, errors="replace") as f:
        return f.read()


def _words(text):
    return set(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", text))


def called_words():
    """every identifier of the test files and of the bindings' function bodies"""
    text = []
    for fn in sorted(os.listdir(TESTS)):
        if fn.endswith(".py") and fn not in ("test_cabi_exports.py", os.path.basename(__file__)):
            text.append(_source(os.path.join(TESTS, fn)))
    for fn in sorted(os.listdir(BINDINGS)):
        if fn.endswith(".py"):
            src = _source(os.path.join(BINDINGS, fn))
            for node in ast.walk(ast.parse(src)):
                if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    text.append(ast.get_source_segment(src, node))
    return _words("\n".join(text))


def defining_source(name):
    """the text of the csrc file that defines the exported function `name` (its name at the start of a line, then its arguments)"""
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".cpp", ".hip", ".c")):
            src = _source(os.path.join(CSRC, fn))
            m = re.search(r"^%s\(" % re.escape(name), src, flags=re.M)
            if m and src.find("{", m.end()) >= 0 and ";" not in src[m.end():src.find("{", m.end())]:
                return src
    return None


def test_every_exported_function_is_reached_by_a_test():
    words = called_words()
    missing = sorted(n for n in ddn.PROTOTYPES if n not in words and n not in REACHED_THROUGH)
    assert not missing, missing


def test_reached_through_entries_hold():
    words = called_words()
    for callee, caller in sorted(REACHED_THROUGH.items()):
        assert callee in ddn.PROTOTYPES and caller in ddn.PROTOTYPES, (callee, caller)
        assert caller in words, "%s: its caller %s is reached by no test" % (callee, caller)
        src = defining_source(caller)
        assert src is not None, "%s is defined in no source file" % caller
        body = re.sub(r"^%s\(" % re.escape(callee), "", src, flags=re.M)              # (the callee's own definition does not count)
        assert callee in _words(body), "%s does not occur in the file that defines %s" % (callee, caller)
    stale = sorted(n for n in REACHED_THROUGH if n in words)
    assert not stale, "called by a test now - drop from REACHED_THROUGH: %s" % stale


def test_no_reset_and_no_drop_in_hides_behind_another_entry_point():
    """the object resets and the single-stream drop-ins under the reference's names are product surface of their own: each has a
    direct test"""
    hidden = [n for n in REACHED_THROUGH if n.endswith("_reset") or not n.startswith("ddn_")]
    assert not hidden, hidden
