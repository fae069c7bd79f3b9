"""Writes tests/golden/dmr_ms_vectors.json: the counts and index assertions the reference's own MS / direct-mode test holds, as numbers.
No source text of the reference is copied: the file holds integers parsed out of

  tests/protocol/dmr/test_dmr_ms_data.c:385-416   dmrMSData(): symbols read behind the sync, which payload entries are the hand-over's
                                                  ends and the live half's ends, the reliabilities of the live half's ends
  tests/protocol/dmr/test_dmr_ms_data.c:442-491   dmrMS() alone: voice syncs, vocoder calls, skips and their total, symbols read
  tests/protocol/dmr/test_dmr_ms_data.c:512-544   dmrMSBootstrap(): the same with the bootstrap burst in front

    python tests/golden/make_golden_dmr_ms.py /path/to/reference"""
import json
import os
import re
import sys


def function_body(text, name):
    at = text.index(name + "(void) {")
    return text[at:text.index("\n}\n", at)]


def asserted(body, name):
    return int(re.search(r"assert\(%s == (\d+)U?\)" % re.escape(name), body).group(1))


def main():
    text = open(os.path.join(sys.argv[1], "tests", "protocol", "dmr", "test_dmr_ms_data.c")).read()
    data = function_body(text, "test_ms_data_collects_payload_and_cleans_state")
    # g_data_sync_payload[a] == payload[b] / g_stream[b]: where the 144 dibits of the burst come from
    cached = [[int(a), int(b)] for a, b in re.findall(r"g_data_sync_payload\[(\d+)\] == payload\[(\d+)\]", data)]
    live = [[int(a), int(b)] for a, b in re.findall(r"g_data_sync_payload\[(\d+)\] == g_stream\[(\d+)\]", data)]
    rel = [[int(a), int(b)] for a, b in re.findall(r"g_data_sync_reliability\[(\d+)\] == (\d+)U", data)]
    base, mod = (int(v) for v in re.search(r"reliability = \(uint8_t\)\((\d+)U \+ \(index % (\d+)U\)\)", text).groups())
    assert len(cached) == 2 and len(live) == 2 and len(rel) == 2
    cyc = function_body(text, "test_ms_voice_cycle_processes_frames_and_cleans_mode_state")
    boot = function_body(text, "test_ms_bootstrap_uses_cached_payload_then_enters_voice_cycle")
    keys = dict(voice_syncs="g_voice_sync_calls", vocoder_calls="g_process_mbe_calls", skips="g_skip_calls", skip_total="g_skip_total",
                symbols="g_stream_index")
    out = dict(data=dict(symbols=asserted(data, "g_stream_index"), data_sync_calls=asserted(data, "g_data_sync_calls"),
                         stereo=asserted(data, "g_data_sync_stereo"), ms_mode=asserted(data, "g_data_sync_ms_mode"), payload_from_handover=cached,
                         payload_from_stream=live, live_reliability=[[a, (r - base) % mod] for a, r in rel]),
               cycle={k: asserted(cyc, v) for k, v in keys.items()}, bootstrap={k: asserted(boot, v) for k, v in keys.items()})
    out["cycle"]["embedded_lc_calls"] = asserted(cyc, "g_data_burst_calls")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dmr_ms_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
