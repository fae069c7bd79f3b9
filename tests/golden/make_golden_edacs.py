#!/usr/bin/env python3
"""Writes tests/golden/edacs_vectors.json: the EDACS data vectors of the reference (numbers and strings only, no source text).

  bch           tests/protocol/edacs/test_edacs_bch.c: the five message -> codeword pairs of edacs_bch(), and its rule that bits of
                the message above bit 27 are ignored (the message pair it compares)
  sync_words    include/dsd-neo/core/sync_patterns.h:107-108: EDACS_SYNC and INV_EDACS_SYNC, with the type each is accepted as
                (frame_sync_try_provoice(): EDACS_SYNC -> DSD_SYNC_EDACS_NEG, INV_EDACS_SYNC -> DSD_SYNC_EDACS_POS; synctype_ids.h)
  dotting       sync_patterns.h:88-89: DOTTING_SEQUENCE_A / _B (no-ops outside a trunk tune)

Run where the reference tree exists: python3 tests/golden/make_golden_edacs.py <reference root>."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_edacs.py <reference root>")
    root = sys.argv[1]
    t = open(os.path.join(root, "tests", "protocol", "edacs", "test_edacs_bch.c")).read()
    body = re.search(r"cases\[\]\s*=\s*\{(.*?)\};", t, re.S).group(1)
    pairs = [[int(a, 16), int(b, 16)] for a, b in re.findall(r"\{\s*0x([0-9A-Fa-f]+)U\s*,\s*0x([0-9A-Fa-f]+)ULL\s*\}", body)]
    assert len(pairs) == 5, pairs
    ign = re.search(r"edacs_bch\(0x([0-9A-Fa-f]+)U\)\s*==\s*edacs_bch\(0x([0-9A-Fa-f]+)U\)", t)
    above = [int(ign.group(1), 16), int(ign.group(2), 16)]
    pats = open(os.path.join(root, "include", "dsd-neo", "core", "sync_patterns.h")).read()
    ids = open(os.path.join(root, "include", "dsd-neo", "core", "synctype_ids.h")).read()
    words = {}
    for name, tname in (("EDACS_SYNC", "EDACS_NEG"), ("INV_EDACS_SYNC", "EDACS_POS")):
        s = re.search(r"#define %s\s+\"([13]{48})\"" % name, pats).group(1)
        words[name] = {"symbols": s, "type": int(re.search(r"#define DSD_SYNC_%s\s+(\d+)" % tname, ids).group(1))}
    dot = {n: re.search(r"#define %s\s+\"([13]{48})\"" % n, pats).group(1) for n in ("DOTTING_SEQUENCE_A", "DOTTING_SEQUENCE_B")}
    out = {"bch": pairs, "bch_ignores_above_28": above, "sync_words": words, "dotting": dot}
    with open(os.path.join(HERE, "edacs_vectors.json"), "w") as f:
        json.dump(out, f, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
