"""Writes tests/golden/nxdn_ctrl_vectors.json: the answers the reference's own NXDN tests hold, as numbers.  No source text of the
reference is copied: the file holds bit patterns (generated here from the coefficients the tests' formulas carry), expected values and
argument tuples, all parsed out of

  tests/protocol/nxdn/test_nxdn_deperm_primitives.c:260-311   crc16cac of nothing and of two patterns; nxdn_sacch_part_of_frame; the RAN
                                                               of a trellis row
  tests/protocol/nxdn/test_nxdn_deperm_windows.c:78-104        the CRC15 windows of a FACCH2 / UDCH row (payload bits 0..183, check field
                                                               bits 184..198, the nine bits behind ignored)
  tests/protocol/nxdn/test_nxdn_deperm_windows.c:158-167       the SACCH segment sequence rule

    python tests/golden/make_golden_nxdn_ctrl.py /path/to/reference"""
import json
import os
import re
import sys


def function_body(text, name):
    at = text.index(name + "(void) {")
    return text[at:text.index("\n}\n", at)]


def pattern(body, name):
    """`name[i] = (uint8_t)((i * aU + bU) & 1U)` over sizeof(name) -> the bits"""
    n = int(re.search(r"uint8_t %s\[(\d+)\]" % name, body).group(1))
    a, b = (int(v) for v in re.search(r"%s\[i\] = \(uint8_t\)\(\(i \* (\d+)U \+ (\d+)U\) & 1U\)" % name, body).groups())
    return [(i * a + b) & 1 for i in range(n)]


def main():
    ref = sys.argv[1]
    prim = open(os.path.join(ref, "tests", "protocol", "nxdn", "test_nxdn_deperm_primitives.c")).read()
    wind = open(os.path.join(ref, "tests", "protocol", "nxdn", "test_nxdn_deperm_windows.c")).read()
    crc = function_body(prim, "test_crc_helpers")
    literal = re.search(r"pattern8\[8\] = \{([^}]*)\}", crc).group(1)
    inputs = dict(empty=[], pattern8=[int(v.strip().rstrip("U")) for v in literal.split(",")], pattern171=pattern(crc, "pattern171"))
    crc16cac = []
    for m in re.finditer(r"crc16cac\((\w+), [^;]*?\), (0x[0-9A-F]+)U\);", crc):
        crc16cac.append(dict(name=m.group(1), bits=inputs[m.group(1)], n=0 if m.group(1) == "empty" else len(inputs[m.group(1)]),
                             crc=int(m.group(2), 16)))
    assert len(crc16cac) == 3, crc16cac
    state = function_body(prim, "test_bit_window_and_state_helpers")
    parts = [dict(sf=int(m.group(1)), part=int(m.group(2))) for m in re.finditer(r"nxdn_sacch_part_of_frame\((\d)U\), (\d)U\)", state)]
    assert len(parts) == 4
    ones = [int(v) for v in re.findall(r"trellis\[(\d)\] = 1U;", state)]
    ran = dict(ones=ones, ran=int(re.search(r"nxdn_ran_from_trellis\(trellis\), (0x[0-9A-F]+)U\)", state).group(1), 16))
    f2 = function_body(wind, "test_facch2_crc15_windows")
    m = re.search(r"for \(size_t i = 0U; i < (\d+)U; i\+\+\) \{\s*trellis_bits\[i\] = \(uint8_t\)\(\(\(i \* (\d+)U\) \+ \(i / (\d+)U\) \+ (\d+)U\) & 1U\);", f2)
    n, a, d, b = (int(v) for v in m.groups())
    crc_at, crc_len = (int(v) for v in re.search(r"write_bits_u16\(trellis_bits, (\d+)U, crc, (\d+)U\)", f2).groups())
    tail_at, tail, tail_len = re.search(r"write_bits_u16\(trellis_bits, (\d+)U, (0x[0-9A-F]+)U, (\d+)U\)", f2).groups()
    windows = dict(payload=[(i * a + i // d + b) & 1 for i in range(n)], check_at=crc_at, check_len=crc_len, tail_at=int(tail_at),
                   tail=int(tail, 16), tail_len=int(tail_len), row=int(re.search(r"trellis_bits\[(\d+)\];", f2).group(1)))
    seq = function_body(wind, "test_sacch_segment_sequence")
    rule = [dict(crc_ok=int(m.group(1)), previous=int(m.group(2)), part=int(m.group(3)), valid=int(m.group(4)))
            for m in re.finditer(r"nxdn_sacch_segment_sequence_is_valid\((\d)U, (\d), (\d)\), (\d)\)", seq)]
    assert len(rule) == 6
    out = dict(crc16cac=crc16cac, part_of_frame=parts, ran_from_trellis=ran, crc15_windows=windows, sequence_rule=rule)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nxdn_ctrl_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
