#!/usr/bin/env python3
"""Writes tests/golden/framesync_vectors.json: the frame-sync known answers of the reference's unit tests (numbers and sync-word
strings only, no source text).

  m17           tests/dsp/test_frame_sync_m17.c:370-390: the eleven M17 transitions (starting lastsynctype and polarity, the
                pattern(s) fed from a cold getFrameSync(), the sync each returns; -1 = none).  The fake reader feeds the pattern at
                10 samples per symbol (+-3), then fill: '1' when a sync is expected, '3' when none is.
  m17_tolerance tests/dsp/test_frame_sync_internal_helpers.c:844-867, the M17-only half: the preamble with its first symbol
                flipped is still the preamble
  m17_levels    test_frame_sync_internal_helpers.c:870-888: the 8-symbol preamble at +-3 through the short window (msize 1)
                -> the preamble, min -1.5, max +1.5
  dmr_rc        test_frame_sync_internal_helpers.c:719-760: the MS reverse-channel word and its complement under both polarities
  cqpsk         tests/dsp/test_frame_sync_p25p2_rtl.c:468-508: the seven CQPSK sync cases, the raw pattern built through the map
                tables (dsd_p25_cqpsk_raw_dibit_for_corrected), the expected type, map index, centre and (max + min) / 2
  cqpsk_neg     test_frame_sync_p25p2_rtl.c:376-422: under P25P2_NEG with map X2400, input 1.0 -> dibit 1, LLR signs (bit0 0, bit1 1)

Sync types are synctype_ids.h values (the reference's numbering; this project adds 1).

Run where the reference tree exists: python3 tests/golden/make_golden_framesync.py [reference root]."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    inc = os.path.join(root, "include", "dsd-neo", "core")
    words = dict(re.findall(r"#define\s+([A-Z0-9_]+)\s+\"([0-3]+)\"", open(os.path.join(inc, "sync_patterns.h")).read()))
    ids = {k: int(v) for k, v in re.findall(r"#define\s+(DSD_SYNC_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", open(os.path.join(inc, "synctype_ids.h")).read())}
    mtxt = open(os.path.join(inc, "p25_cqpsk_dibit.h")).read()
    map_ids = {k: int(v) for k, v in re.findall(r"#define\s+DSD_P25_CQPSK_DIBIT_MAP_([A-Z0-9]+)\s+(\d+)u", mtxt)}
    body = mtxt[mtxt.index("maps[DSD_P25_CQPSK_DIBIT_MAP_COUNT][4]"):]
    maps = [[int(x) for x in row.split(",")] for row in re.findall(r"\{(\d, \d, \d, \d)\}", body)[:5]]
    assert len(maps) == 5, maps

    def sync_id(name):
        return ids[name]

    def raw_for_corrected(m, corrected):   # the first raw dibit the map corrects to `corrected`
        for raw in range(4):
            if maps[m][raw] == corrected:
                return raw
        return corrected

    def pattern(expr):   # "M17_PRE M17_PRE" -> the concatenated words
        return "".join(words[w] for w in expr.split())

    # ---- M17 transitions
    t = open(os.path.join(root, "tests", "dsp", "test_frame_sync_m17.c")).read()
    main_body = t[t.index("main(void)"):]
    m17 = []
    for m in re.finditer(r"run_m17_sync_case\((DSD_SYNC_[A-Z0-9_]+), (\d)U, ([A-Z0-9_]+), (-1|DSD_SYNC_[A-Z0-9_]+),\s*\"([^\"]+)\"\)", main_body):
        m17.append({"label": m.group(5), "last": sync_id(m.group(1)), "polarity": int(m.group(2)),
                    "steps": [{"pattern": pattern(m.group(3)), "expect": -1 if m.group(4) == "-1" else sync_id(m.group(4))}]})
    for m in re.finditer(r"run_m17_two_step_case\(([A-Z0-9_ ]+), (DSD_SYNC_[A-Z0-9_]+), ([A-Z0-9_]+), (-1|DSD_SYNC_[A-Z0-9_]+),"
                         r"\s*\"([^\"]+)\"\)", main_body):
        m17.append({"label": m.group(5), "last": sync_id("DSD_SYNC_NONE"), "polarity": 0,
                    "steps": [{"pattern": pattern(m.group(1)), "expect": sync_id(m.group(2))},
                              {"pattern": pattern(m.group(3)), "expect": -1 if m.group(4) == "-1" else sync_id(m.group(4))}]})
    assert len(m17) == 11, len(m17)
    sps = int(re.search(r"samples_per_symbol = (\d+)U;", t).group(1))

    # ---- helpers file: the M17-only preamble tolerance, the short-window levels, DMR RC
    h = open(os.path.join(root, "tests", "dsp", "test_frame_sync_internal_helpers.c")).read()
    tol = h[h.index("test_m17_auto_preamble_disambiguation_preserves_forced_tolerance(void)"):]
    tol = tol[:tol.index("opts.frame_dmr = 1;")]
    assert "one_error_preamble[0] = one_error_preamble[0] == '1' ? '3' : '1';" in tol
    pre = words["M17_PRE"]
    one_err = ("3" if pre[0] == "1" else "1") + pre[1:]
    exp = re.search(r"one_error_preamble, 8\) == (DSD_SYNC_[A-Z0-9_]+)\);", tol).group(1)
    m17_tol = {"pattern": one_err, "expect": sync_id(exp)}
    lv = h[h.index("test_short_m17_window_estimates_levels_without_warm_start_history(void)"):]
    lv = lv[:lv.index("\n}\n")]
    assert "opts.msize = 1;" in lv
    levels = [-3.0 if c == "3" else 3.0 for c in pre]
    m17_lv = {"pattern": pre, "levels": levels, "msize": 1,
              "expect": sync_id(re.search(r"levels, 8\) == (DSD_SYNC_[A-Z0-9_]+)\);", lv).group(1)),
              "min": float(re.search(r"state\.min - \((-?[\d.]+)f\)", lv).group(1)),
              "max": float(re.search(r"state\.max - ([\d.]+)f\)", lv).group(1))}
    rc = h[h.index("test_dmr_rc_sync_matches_and_respects_polarity(void)"):]
    rc = rc[:rc.index("/* No DMR decoding")]
    dmr_rc, inverted = [], 0
    for m in re.finditer(r"opts\.inverted_dmr = (\d);|reset\(&opts, &state\);|try_protocol_matches\(&opts, &state, ([A-Z0-9_]+), 24\) == "
                         r"(DSD_SYNC_[A-Z0-9_]+)\)", rc):
        if m.group(0).startswith("reset"):
            inverted = 0
        elif m.group(1) is not None:
            inverted = int(m.group(1))
        else:
            dmr_rc.append({"inverted": inverted, "word": m.group(2), "pattern": words[m.group(2)], "expect": sync_id(m.group(3))})
    assert len(dmr_rc) == 4, dmr_rc

    # ---- CQPSK
    p = open(os.path.join(root, "tests", "dsp", "test_frame_sync_p25p2_rtl.c")).read()
    pm = p[p.index("main(void)"):]
    cq, pending = [], None
    for m in re.finditer(r"build_raw_pattern_for_map\(([A-Z0-9_]+), DSD_P25_CQPSK_DIBIT_MAP_([A-Z0-9]+), rotated|"
                         r"run_(p25p2|p25p1)_sync_case\(([A-Za-z0-9_]+), (DSD_SYNC_[A-Z0-9_]+), DSD_P25_CQPSK_DIBIT_MAP_([A-Z0-9]+),\s*"
                         r"\"([^\"]+)\"\)", pm):
        if m.group(1):
            pending = (m.group(1), map_ids[m.group(2)])
            continue
        corrected = pending[0] if m.group(4) == "rotated" else m.group(4)
        build_map = pending[1] if m.group(4) == "rotated" else map_ids["IDENTITY"]
        raw = "".join(str(raw_for_corrected(build_map, int(c))) for c in words[corrected])
        cq.append({"label": m.group(7), "protocol": m.group(3), "corrected": words[corrected], "pattern": raw,
                   "expect": sync_id(m.group(5)), "map": map_ids[m.group(6)], "center": 0.0, "scanner_center": 0.0})
        pending = None
    assert len(cq) == 7, cq
    assert "return run_p25_sync_case(pattern, 0, 1, expected_sync, expected_map, 0.0f, label);" in p
    neg = p[p.index("test_negative_cqpsk_dibit_polarity(void)"):]
    neg = neg[:neg.index("\n}\n")]
    cq_neg = {"synctype": sync_id(re.search(r"state\.synctype = (DSD_SYNC_[A-Z0-9_]+);", neg).group(1)),
              "map": map_ids[re.search(r"DIBIT_MAP_([A-Z0-9]+);", neg).group(1)],
              "input": float(re.search(r"digitize\(&opts, &state, ([\d.]+)f\)", neg).group(1)),
              "dibit": int(re.search(r"got != (\d)", neg).group(1)),
              "llr_bits": [int(x) for x in re.search(r"llr_matches_bit\(soft\.llr\[0\], (\d)\) \|\| !llr_matches_bit\(soft\.llr\[1\], (\d)\)",
                                                     neg).groups()]}

    out = {"sync_ids": {k[9:]: v for k, v in ids.items() if k.startswith("DSD_SYNC_") and not k.startswith("DSD_SYNC_IS")},
           "m17_words": {k: words[k] for k in ("M17_PRE", "M17_PIV", "M17_LSF", "M17_STR", "M17_BRT", "M17_PKT", "M17_EOT", "M17_EOT_INV")},
           "m17_samples_per_symbol": sps, "m17": m17, "m17_tolerance": m17_tol, "m17_levels": m17_lv, "dmr_rc": dmr_rc,
           "cqpsk_maps": maps, "cqpsk": cq, "cqpsk_neg": cq_neg}
    with open(os.path.join(HERE, "framesync_vectors.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
