#!/usr/bin/env python3
"""Writes tests/golden/dstar_vectors.json: the D-STAR tables and the data vectors of the reference's D-STAR unit tests (numbers and
strings only, no source text).

  interleave_w / interleave_x   include/dsd-neo/protocol/dstar/dstar_const.h: the 72-entry AMBE frame schedule (dibit i of a voice
                                frame -> ambe_fr[w[i]][x[i]])
  sd_scrambler                  src/protocol/dstar/dstar_slow_data.c:27 (the 24-bit slow-data pattern, 0x0EF2C9)
  sync_words                    include/dsd-neo/core/sync_patterns.h:44-47 with their type ids (synctype_ids.h:44-47)
  header                        tests/protocol/dstar/test_dstar_header_utils.c: the round-trip info bits, the encoded-header fixture
                                (flags 0x78 / 0x80, the four callsign fields) and what the call state reports, the CRC check value
  sd_header / sd_text           the same file: the slow-data header in wire CRC order, the text byte after the marker
  process                       tests/protocol/dstar/test_dstar_process.c: dibit counts, the stub's dibit rule (call number & 3) and
                                soft-symbol rule (call number + 1 times a step), the first AMBE frame's checked cells, the slow data
                                expected after the first voice frame, the first and last header soft symbols
  dispatch                      tests/protocol/dstar/test_dstar_sync_dispatch.c: which sync types run the voice or header path

Run where the reference tree exists: python3 tests/golden/make_golden_dstar.py [reference root]."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def ints_of(txt, name):
    m = re.search(r"%s\[\w*\]\s*=\s*\{(.*?)\};" % name, txt, re.S)
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return [int(x, 0) for x in re.findall(r"0x[0-9A-Fa-f]+|\d+", body)]


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    const = open(os.path.join(root, "include", "dsd-neo", "protocol", "dstar", "dstar_const.h")).read()
    w, x = ints_of(const, "dstar_interleave_w"), ints_of(const, "dstar_interleave_x")
    assert len(w) == 72 and len(x) == 72 and sorted(zip(w, x)) == sorted(set(zip(w, x)))
    sdc = open(os.path.join(root, "src", "protocol", "dstar", "dstar_slow_data.c")).read()
    sd = ints_of(sdc, "sd_d")
    assert len(sd) == 24
    pats = open(os.path.join(root, "include", "dsd-neo", "core", "sync_patterns.h")).read()
    ids = open(os.path.join(root, "include", "dsd-neo", "core", "synctype_ids.h")).read()
    words = {}
    for name, tname in (("DSTAR_SYNC", "DSTAR_VOICE_POS"), ("INV_DSTAR_SYNC", "DSTAR_VOICE_NEG"), ("DSTAR_HD", "DSTAR_HD_POS"),
                        ("INV_DSTAR_HD", "DSTAR_HD_NEG")):
        s = re.search(r"#define %s\s+\"([13]{24})\"" % name, pats).group(1)
        t = int(re.search(r"#define DSD_SYNC_%s\s+(\d+)" % tname, ids).group(1))
        words[name] = {"symbols": s, "type": t}

    d = os.path.join(root, "tests", "protocol", "dstar")
    hu = open(os.path.join(d, "test_dstar_header_utils.c")).read()
    sc = ints_of(hu, "k_slow_data_scrambler")
    assert sc == sd
    m = re.search(r"info_bits\[i\] = \(int\)\(\(i \* (\d+) \+ (\d+)\) & 0x1\);", hu)
    so = re.search(r"soft_interleaved\[i\] = interleaved\[i\] \? 0x([0-9A-Fa-f]+)U : 0x([0-9A-Fa-f]+)U;", hu)
    roundtrip = {"mul": int(m.group(1)), "add": int(m.group(2)), "soft_one": int(so.group(1), 16), "soft_zero": int(so.group(2), 16)}
    fix = hu[hu.index("build_encoded_header_fixture(float"):]
    fields = re.findall(r"DSD_MEMCPY\(header \+ (\d+), \"([^\"]*)\", (\d+)\);", fix)
    fixture = {"fields": [[int(a), s, int(n)] for a, s, n in fields]}
    flags = [int(v, 16) for v in re.findall(r"build_encoded_header_fixture\(soft_rx, 0x([0-9A-Fa-f]+)U\);", hu)]
    kinds = re.findall(r"call\.kind == DSD_CALL_KIND_(VOICE|DATA)", hu)[:2]
    want = re.findall(r"strcmp\(call\.(route_text\[1\]|route_text\[0\]|target_text|source_text), \"([^\"]*)\"\)", hu)[:4]
    names = {"route_text[1]": "rpt2", "route_text[0]": "rpt1", "target_text": "dst", "source_text": "src"}
    fixture["cases"] = [{"flags": f, "kind": k.lower()} for f, k in zip(flags, kinds)]
    fixture["call"] = {names[a]: b for a, b in want}
    crc = re.search(r"const uint8_t payload\[\] = \"([^\"]*)\";\s*//[^\n]*\n\s*assert\(dstar_crc16\(payload, sizeof\(payload\) - 1\) == 0x([0-9a-fA-F]+)\);",
                    hu)
    crc_vec = {"text": crc.group(1), "crc": int(crc.group(2), 16)}
    a = hu.index("test_slow_data_header_accepts_wire_crc_order(void) {")
    body = hu[a:hu.index("pack_slow_data_bytes(const uint8_t bytes[60]", a)]
    cfields = re.findall(r"DSD_MEMCPY\(compact \+ (\d+), \"([^\"]*)\", (\d+)\);", body)
    cbytes = re.findall(r"compact\[(\d+)\] = 0x([0-9A-Fa-f]+);", body)
    sd_header = {"marker": int(re.search(r"bytes\[0\] = 0x([0-9A-Fa-f]+);", body).group(1), 16), "fill": 0x20,
                 "fields": [[int(a), s, int(n)] for a, s, n in cfields], "bytes": [[int(a), int(v, 16)] for a, v in cbytes]}
    a = hu.index("test_slow_data_text_keeps_byte_after_marker(void) {")
    body = hu[a:hu.index("test_slow_data_aprs_latitude", a)]
    tb = [[int(a), int(v, 16)] for a, v in re.findall(r"bytes\[(\d+)\] = 0x([0-9A-Fa-f]+);", body)]
    tb += [[int(a), ord(c)] for a, c in re.findall(r"bytes\[(\d+)\] = '(.)';", body)]
    tw = [[int(a), c] for a, c in re.findall(r"state\.dstar_txt\[(\d+)\] == '(.)'", body)]
    sd_text = {"fill": 0x20, "bytes": sorted(tb), "text_at": tw}

    pr = open(os.path.join(d, "test_dstar_process.c")).read()
    enum = {k: int(v) for k, v in re.findall(r"(DSTAR_\w+) = (\d+),", pr)}
    cells = [[int(a), int(b), int(v)] for a, b, v in re.findall(r"captured_ambe_frame\[(\d+)\]\[(\d+)\] == (\d+)\)", pr)]
    step = float(re.search(r"\*out_soft_symbol = \(float\)\(soft_symbol_calls \+ 1\) \* ([0-9.]+)F;", pr).group(1))
    mask = int(re.search(r"int value = dibit_calls & (\d+);", pr).group(1))
    sdx = re.search(r"int expected = \((\w+) \+ i\) & (\d+);", pr)
    hdr_first = float(re.search(r"captured_soft_symbols\[0\] == ([0-9.]+)F", pr).group(1))
    hdr_last = float(re.search(r"captured_soft_symbols\[DSD_DSTAR_HEADER_CODED_BITS - 1\] == ([0-9.]+)F", pr).group(1))
    process = {"voice_frames": enum["DSTAR_VOICE_FRAMES"], "voice_dibits": enum["DSTAR_VOICE_DIBITS_PER_FRAME"],
               "slow_frames": enum["DSTAR_SLOW_DATA_FRAMES"], "slow_dibits": enum["DSTAR_SLOW_DATA_DIBITS_PER_FRAME"],
               "dibit_mask": mask, "ambe_cells": cells, "slow_data_first": {"offset": enum[sdx.group(1)], "mask": int(sdx.group(2))},
               "header_soft": {"step": step, "first": hdr_first, "last": hdr_last}}
    ds = open(os.path.join(d, "test_dstar_sync_dispatch.c")).read()
    voice = re.search(r"voice_synctypes\[\] = \{(.*?)\};", ds).group(1)
    header = re.search(r"header_synctypes\[\] = \{(.*?)\};", ds).group(1)
    tid = lambda s: [int(re.search(r"#define %s\s+(\d+)" % n, ids).group(1)) for n in re.findall(r"DSD_SYNC_\w+", s)]
    dispatch = {"voice": tid(voice), "header": tid(header)}

    out = {"interleave_w": w, "interleave_x": x, "sd_scrambler": sd, "sync_words": words, "header_roundtrip": roundtrip,
           "header_fixture": fixture, "crc16": crc_vec, "sd_header": sd_header, "sd_text": sd_text, "process": process, "dispatch": dispatch}
    with open(os.path.join(HERE, "dstar_vectors.json"), "w") as f:
        json.dump(out, f)
    print("wrote dstar_vectors.json:", len(cells), "AMBE cells,", len(fixture["cases"]), "header fixtures")


if __name__ == "__main__":
    main()
