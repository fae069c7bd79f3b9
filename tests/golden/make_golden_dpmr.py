#!/usr/bin/env python3
"""Writes tests/golden/dpmr_vectors.json: the data vectors of the reference's dPMR unit tests (numbers only, no source text).

  color_codes   tests/protocol/dpmr/test_dpmr_color_code.c: the 64 (24-bit channel code, colour code) pairs; the same pairs
                with the dibit LSBs cleared must map alike (mask 0x555555); 0x000000 is rejected (-1)
  scrambler     tests/protocol/dpmr/test_dpmr_scrambler.c: 72 zero bits through the x^9 + x^5 + 1 LFSR seeded 0x1FF -> the 72
                output bits and the advanced state
  crc7 / cch_crc / aiid   tests/protocol/dpmr/test_dpmr_voice_bridge.c:236-258
  superframe_parts        test_dpmr_voice_bridge.c:261-334 (called / calling IDs, weak IDs, the next-part toggle)
  voice_halves            test_dpmr_voice_bridge.c:118-190 (which halves are synthesised, muted without a key)

Run where the reference tree exists: python3 tests/golden/make_golden_dpmr.py [reference root]."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    d = os.path.join(root, "tests", "protocol", "dpmr")
    cc_txt = open(os.path.join(d, "test_dpmr_color_code.c")).read()
    pairs = [(int(a, 16), int(b)) for a, b in re.findall(r"\{0x([0-9A-Fa-f]{6})u,\s*(\d+)\}", cc_txt)]
    assert len(pairs) == 64 and sorted(p[1] for p in pairs) == list(range(64)), len(pairs)
    sc_txt = open(os.path.join(d, "test_dpmr_scrambler.c")).read()
    m = re.search(r"expected\[72\] = \{(.*?)\};", sc_txt, re.S)
    bits = [int(x) for x in re.findall(r"\d", m.group(1))]
    state = int(re.search(r"dpmr-scrambler-advanced-state\", lfsr, 0x([0-9A-Fa-f]+)U", sc_txt).group(1), 16)
    assert len(bits) == 72
    vb = open(os.path.join(d, "test_dpmr_voice_bridge.c")).read()
    crc_in = [int(x) for x in re.findall(r"\d", re.search(r"crc_bits\[12\] = \{(.*?)\};", vb, re.S).group(1))]
    crc_out = int(re.search(r"\"crc7-pattern\", dpmr_crc7\(crc_bits, 12U\), 0x([0-9A-Fa-f]+)", vb).group(1), 16)
    set_bits = [int(x) for x in re.findall(r"cch_bits\[(\d+)\] = 1U;", vb)]
    cch_crc = int(re.search(r"\"cch-crc-extract\", dpmr_extract_cch_crc\(cch_bits\), 0x([0-9A-Fa-f]+)", vb).group(1), 16)
    ids = re.findall(r"dpmr_convert_air_interface_id\((\d+)U, id\);\s*rc \|= expect_int\(\"[^\"]+\", strcmp\(id, \"([0-9*]{7})\"\)", vb)
    assert len(ids) >= 4
    # superframe-part outcomes (:261-334): each step is a part (frame numbers, ID, CRC / Hamming verdicts) fed to
    # dpmr_update_superframe_part(), optionally after a forced next-part value, and the call state's called / calling ID and
    # next-part value after it ("" = not checked)
    body = vb[vb.index("test_superframe_part_updates_called_and_calling_ids"):vb.index("test_id_print_side_effects")]
    steps, forced = [], None
    for m in re.finditer(r"opts\.dPMR_next_part_of_superframe = (\d+);|part = \(dpmr_superframe_part\)\{(.*?)\};|"
                         r"dpmr_update_superframe_part\(&opts, &state, &part\);|expect_int\(\"([a-z-]+)\", (.*?), (-?\d+)\);", body, re.S):
        if m.group(1) is not None:
            forced = int(m.group(1))
        elif m.group(2) is not None:
            nums = [int(x) for x in re.findall(r"\d+", m.group(2).replace("true", "1").replace("false", "0"))]
            part = {"fn": nums[0:2], "id": nums[2], "crc_ok": nums[3:5], "ham_ok": [nums[5:7], nums[7:9]]}
        elif m.group(0).startswith("dpmr_update"):
            steps.append({"part": dict(part), "force_next": forced, "expect": {}})
            forced = None
        else:
            got, want = m.group(4), int(m.group(5))
            e = steps[-1]["expect"]
            t = re.search(r"strcmp\(call\.(target|source)_text, \"([0-9*]*)\"\)", got)
            if t and want == 0:
                e["tg" if t.group(1) == "target" else "src"] = t.group(2)
            elif "dPMR_next_part_of_superframe" in got:
                e["next"] = want
    assert len(steps) == 7, len(steps)
    # voice halves (:118-190): the modes / versions of the two CCHs, whether a key is set -> frames synthesised per half, muted
    halves = []
    vbody = vb[vb.index("first-group") - 2000:vb.index("second-group-synctype-restored")]
    for grp in ("first", "second"):
        seg = vbody[:vbody.index("%s-group-mbe-calls" % grp)]
        vbody = vbody[vbody.index("%s-group-mbe-calls" % grp) + 1:]
        seg = seg[seg.rfind("FrameNumbering[0]") - 400:]
        mode = {int(a): int(b) for a, b in re.findall(r"CommunicationMode\[(\d)\] = (\d+);", seg)}
        ver = {int(a): int(b) for a, b in re.findall(r"Version\[(\d)\] = (\d+);", seg)}
        key = 1 if re.search(r"state\.R = 0x[0-9A-Fa-f]+ULL;", seg) else 0
        calls = int(re.search(r"\"%s-group-mbe-calls\", \(int\)g_mbe_calls, (\d+)\)" % grp, vb).group(1))
        muted = int(re.search(r"\"%s-group-(?:final-)?(?:un)?muted\", [a-z_.]*dmr_encL, (\d)\)" % grp, vb).group(1))
        halves.append({"mode": [mode.get(0, 0), mode.get(1, 0)], "version": [ver.get(0, 0), ver.get(1, 0)], "key": key, "frames": calls,
                       "muted": muted})
    out = {"superframe_parts": steps, "voice_halves": halves, "color_codes": pairs, "color_reject": [0], "scrambler": {"seed": 0x1FF, "in_zero_bits": 72, "out": bits, "state": state},
           "crc7": {"bits": crc_in, "crc": crc_out, "empty": 0}, "cch_crc": {"ones_at": set_bits, "crc": cch_crc},
           "aiid": [[int(v), s] for v, s in ids]}
    with open(os.path.join(HERE, "dpmr_vectors.json"), "w") as f:
        json.dump(out, f)
    print("wrote", len(pairs), "colour codes,", len(ids), "AI-ID strings")


if __name__ == "__main__":
    main()
