"""Writes tests/golden/dmr_pdu_vectors.json: vectors that anchor tests/dmr_pdu.py to the reference.  No source text of the reference is
copied: the vectors are numbers, either parsed out of its DMR tests or recorded from a run of its own dmr_block.c.

  profiles      parsed out of tests/protocol/dmr/test_dmr_dburst_profile.c (:387-407): the expected_profile table - data type,
                confirmed, header format -> subtype, CRC mask, flags, CRC length, PDU length, PDU start
  sequences     recorded: a harness (below) is compiled at generation time against the reference's src/protocol/dmr/dmr_block.c,
                dmr_ars.c and dmr_block_crypto.c, with the stubs of tests/protocol/dmr/test_dmr_relaxed_header_ip.c (the harness includes
                that file, its main renamed) and the oracle build for dmr_utils.c / bit_packing.c.  It drives dmr_dheader(),
                dmr_block_assembler() and dmr_reset_blocks() under the default options (aggressive_framesync = 1, dmr_crc_relaxed_default
                = 0) and prints, after every call, the slot's fields, the head of its dmr_pdu_sf row and what was dispatched: the
                reference test's own cases that run under those options (a CRC-valid type 1 PDU in strict mode for SAP 4 / 10 / 2 / 3,
                the UDT ISO7 single block, dmr_reset_blocks()' defaults, the irrecoverable header, the short-data-defined header, the
                type 2 aggregate length refusal) and whole header + block sequences of every rate whose CRC32 trailer the reference
                test's append_type1_crc32 (ComputeCrc32Bit) made, a corrupted one, the MNIS and another proprietary header, an MBC
  crc9          transcribed by hand from test_dmr_confirmed_crc9.c (:30-92 rate 1/2, :95-170 rate 1, :173-222 rate 3/4): DBSN, mask and
                the payload bits its formulas give, the bit it flips; crc9_ref = ComputeCrc9Bit of the oracle build over the span
  type1_bounds  transcribed by hand from test_dmr_block_type1_bounds.c (:36-81): the slot it seeds, the block length, the byte counter
                it expects (cap = the row's 3072 bytes)
  type2_bounds  transcribed by hand from test_dmr_block_type2_bounds.c (:63-78): the UDT block counts it seeds

    python tests/golden/make_golden_dmr_pdu.py /path/to/reference /path/to/oracle/_ref"""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HARNESS = r'''
#define main ref_test_main
#define dmr_cspdu ref_test_cspdu_stub
#include "%(test)s"
#undef main
#undef dmr_cspdu
static int g_cspdu_calls, g_cspdu_crc;
void dmr_cspdu(dsd_opts* opts, dsd_state* state, uint8_t* bits, uint8_t* bytes, uint32_t crc, uint32_t errs) {
    (void)opts; (void)state; (void)bits; (void)bytes; (void)errs;
    g_cspdu_calls++;
    g_cspdu_crc = (int)crc;
}
static dsd_opts opts;
static dsd_state state;
static Event_History_I history[2];
static const char* scen;
static int step;
static void hex(const char* key, const uint8_t* p, int n) {
    printf("\"%%s\": \"", key);
    for (int i = 0; i < n; i++) printf("%%02x", p[i]);
    printf("\"");
}
static void dump(const char* op, int slot, const uint8_t* in, int n, int a, int b) {
    printf("{\"scenario\": \"%%s\", \"step\": %%d, \"op\": \"%%s\", \"slot\": %%d, \"a\": %%d, \"b\": %%d, ", scen, step++, op, slot, a, b);
    hex("input", in, n);
    printf(", \"dispatched\": %%d, \"cspdu\": %%d, \"cspdu_crc\": %%d, \"state\": [", (int)(g_decode_ip_calls + g_sd_pdu_calls + g_udp_comp_calls + g_datacall_calls),
           g_cspdu_calls, g_cspdu_crc);
    for (int s = 0; s < 2; s++) {
        printf("{\"hfmt\": %%d, \"sap\": %%d, \"blocks\": %%d, \"counter\": %%d, \"conf\": %%d, \"hvalid\": %%d, \"p_head\": %%d, \"poc\": %%d, \"byte_ctr\": %%d, "
               "\"dbsn_have\": %%d, \"dbsn_exp\": %%d, \"udt_res\": %%d, \"crc_valid0\": %%d, \"src\": %%llu, \"tgt\": %%llu, \"gi\": %%d, ",
               state.data_header_format[s], state.data_header_sap[s], state.data_header_blocks[s], state.data_block_counter[s], state.data_conf_data[s],
               state.data_header_valid[s], state.data_p_head[s], state.data_block_poc[s], state.data_byte_ctr[s], state.data_dbsn_have[s],
               state.data_dbsn_expected[s], state.udt_uab_reserved[s], state.data_block_crc_valid[s][0], state.dmr_lrrp_source[s],
               state.dmr_lrrp_target[s], state.dmr_data_target_is_group[s]);
        hex("sf", state.dmr_pdu_sf[s], 96);
        printf("}%%s", s ? "" : ", ");
    }
    printf("]}\n");
}
static void spies(void) { reset_datacall_spy(); g_cspdu_calls = 0; g_cspdu_crc = -1; }
static void begin(const char* name) {
    scen = name; step = 0;
    memset(&opts, 0, sizeof opts); memset(&state, 0, sizeof state); memset(history, 0, sizeof history);
    state.event_history_s = history;
    opts.aggressive_framesync = 1; opts.dmr_crc_relaxed_default = 0;
    dmr_reset_blocks(&opts, &state);
    spies();
}
static void seeded(int slot) { dump("seed", slot, (const uint8_t*)"", 0, 0, 0); }
static void header(int slot, const uint8_t by[12], int crc, int errs) {
    uint8_t bits[196], b[12];
    memset(bits, 0, sizeof bits); memcpy(b, by, 12);
    for (int i = 0; i < 96; i++) bits[i] = (by[i / 8] >> (7 - i %% 8)) & 1;
    state.currentslot = slot; spies();
    dmr_dheader(&opts, &state, b, bits, (uint32_t)crc, (uint32_t)errs);
    dump("header", slot, by, 12, crc, errs);
}
static void block(int slot, const uint8_t* by, int len, int type) {
    uint8_t b[24];
    memcpy(b, by, len);
    state.currentslot = slot; spies();
    dmr_block_assembler(&opts, &state, b, (uint8_t)len, 0, (uint8_t)type);
    dump("block", slot, by, len, len, type);
}
static void fill(uint8_t* row, int n, int mul, int add) { for (int i = 0; i < n; i++) row[i] = (uint8_t)(mul * i + add); }
static void hdr_bytes(uint8_t by[12], int gi, int a, int dpf, int sap, int poc, uint32_t tgt, uint32_t src, int b8, int b9) {
    memset(by, 0, 12);
    by[0] = (uint8_t)((gi << 7) | (a << 6) | (((poc >> 4) & 1) << 4) | dpf); by[1] = (uint8_t)((sap << 4) | (poc & 15));
    by[2] = tgt >> 16; by[3] = tgt >> 8; by[4] = tgt; by[5] = src >> 16; by[6] = src >> 8; by[7] = src; by[8] = (uint8_t)b8; by[9] = (uint8_t)b9;
}
static void type1_seed(int slot, int blocks, int fmt, int sap, int conf, int p_head) {
    state.data_header_valid[slot] = 1; state.data_header_blocks[slot] = blocks; state.data_header_format[slot] = fmt;
    state.data_header_sap[slot] = sap; state.data_block_counter[slot] = 1; state.data_conf_data[slot] = conf; state.data_p_head[slot] = p_head;
    seeded(slot);
}
int main(void) {
    uint8_t row[3 * 24 + 16], by[12], bits[196];
    /* the reference test's own cases */
    { uint8_t b[12] = {0x45, 0x00, 0x00, 0x14, 0x12, 0x34, 0x00, 0x00, 0, 0, 0, 0};
      append_type1_crc32(b, 12); begin("strict_type1_sap4"); type1_seed(0, 1, 2, 4, 0, 0); block(0, b, 12, 1); }
    { uint8_t b[12] = {0x83, 0x10, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77, 0, 0, 0, 0};
      const int saps[3] = {10, 2, 3}; const char* names[3] = {"strict_type1_sap10", "strict_type1_sap2", "strict_type1_sap3"};
      append_type1_crc32(b, 12);
      for (int k = 0; k < 3; k++) { begin(names[k]); type1_seed(0, 1, 2, saps[k], 0, 0); block(0, b, 12, 1); } }
    { uint8_t blk[12]; begin("udt_iso7_single_block");
      build_udt_header(by, bits, 0x03U, 0x000111U, 0x000222U); build_udt_iso7_block(blk, "HELLO");
      header(0, by, 1, 0); state.data_block_crc_valid[0][0] = 1; seeded(0); block(0, blk, 12, 3); }
    { begin("reset_blocks_defaults");
      state.data_block_counter[0] = 42; state.data_block_counter[1] = 43; state.data_header_blocks[0] = 44; state.data_header_blocks[1] = 45;
      state.data_header_format[0] = 2; state.data_header_format[1] = 3; state.data_dbsn_have[0] = 1; state.data_dbsn_expected[0] = 9;
      seeded(0); dmr_reset_blocks(&opts, &state); dump("reset", 0, (const uint8_t*)"", 0, 0, 0); }
    { begin("irrecoverable_header"); memset(by, 0, 12);
      state.data_header_valid[1] = 1; state.data_p_head[1] = 1; state.data_conf_data[1] = 1; state.data_block_counter[1] = 9;
      state.data_header_blocks[1] = 9; state.data_header_format[1] = 2; seeded(1); header(1, by, 0, 1); }
    { begin("short_data_defined_header"); memset(bits, 0, sizeof bits);
      set_bits(bits, 1, 1U, 1); set_bits(bits, 2, 1U, 2); set_bits(bits, 4, 13U, 4); set_bits(bits, 8, 10U, 4); set_bits(bits, 12, 1U, 4);
      set_bits(bits, 16, 0x010203U, 24); set_bits(bits, 40, 0x040506U, 24); set_bits(bits, 64, 18U, 6); set_bits(bits, 72, 7U, 8);
      pack_bits_to_bytes(bits, by, 96); header(0, by, 1, 0); }
    { uint8_t b[12] = {0x80, 0x01, 0x02, 0x03}; begin("type2_aggregate_length_refused");
      state.data_header_valid[0] = 1; state.data_block_counter[0] = 9; state.data_block_crc_valid[0][0] = 1; seeded(0); block(0, b, 12, 2); }
    /* whole sequences: header, then blocks whose row closes with the trailer append_type1_crc32 makes */
    { const int lens[6] = {12, 18, 24, 10, 16, 22};
      const char* names[6] = {"unconfirmed_12", "unconfirmed_18", "unconfirmed_24", "confirmed_10", "confirmed_16", "confirmed_22"};
      for (int k = 0; k < 6; k++) {
          const int conf = k >= 3, n = 3 * lens[k];
          begin(names[k]); fill(row, n, 37, 11 + k); append_type1_crc32(row, n);
          hdr_bytes(by, 1, 0, conf ? 3 : 2, 4, 5, 0x0A0B0C, 0x010203, 0x80 | 3, 0); header(k & 1, by, 1, 0);
          for (int j = 0; j < 3; j++) block(k & 1, row + j * lens[k], lens[k], 1);
      } }
    { begin("confirmed_16_corrupted"); fill(row, 48, 29, 7); append_type1_crc32(row, 48); row[21] ^= 0x10;
      hdr_bytes(by, 0, 0, 3, 4, 0, 0x000010, 0x000020, 3, 0); header(0, by, 1, 0);
      for (int j = 0; j < 3; j++) block(0, row + j * 16, 16, 1); }
    { begin("header_crc_rejected"); hdr_bytes(by, 0, 0, 3, 4, 0, 0x000010, 0x000020, 3, 0);
      state.data_conf_data[0] = 1; state.data_header_blocks[0] = 9; state.data_block_counter[0] = 5; state.data_block_poc[0] = 3; seeded(0);
      header(0, by, 0, 0); }
    { uint8_t ph[12] = {0x1F, 0x10, 0xA1, 0xA2, 0x11, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0, 0};
      begin("mnis_header_offset_12"); hdr_bytes(by, 0, 0, 3, 4, 2, 0x000030, 0x000040, 3, 0); header(1, by, 1, 0); header(1, ph, 1, 0);
      memcpy(row, ph, 10); fill(row + 10, 20, 41, 3); append_type1_crc32(row, 30); row[29] ^= 1; /* the MNIS header waives the CRC32 */
      for (int j = 0; j < 2; j++) block(1, row + 10 + j * 10, 10, 1); }
    { uint8_t ph[12] = {0x4F, 0x68, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x0B, 0x0C, 0, 0};
      begin("other_proprietary_header"); hdr_bytes(by, 0, 0, 2, 4, 0, 0x000050, 0x000060, 0x80 | 3, 0); header(0, by, 1, 0); header(0, ph, 1, 0);
      fill(row, 24, 43, 9); append_type1_crc32(row, 24);
      for (int j = 0; j < 2; j++) block(0, row + j * 12, 12, 1); }
    { begin("response_header"); hdr_bytes(by, 0, 0, 1, 4, 0, 0x000070, 0x000080, 0, 0x08); header(0, by, 1, 0); }
    { uint8_t m[36], mb[8 * 24];
      begin("mbc_two_continuation_blocks"); fill(m, 36, 17, 1); m[0] &= 0x3F; m[12] &= 0x3F; m[24] = (m[24] & 0x3F) | 0x80;
      for (int i = 0; i < 22 * 8; i++) mb[i] = (m[12 + i / 8] >> (7 - i %% 8)) & 1;
      { uint32_t c = dsd_crc_ccitt16_bits(mb, 22 * 8); m[34] = (uint8_t)(c >> 8); m[35] = (uint8_t)c; }
      state.data_block_counter[0] = 0; state.data_header_valid[0] = 1; state.data_block_crc_valid[0][0] = 1; seeded(0); /* as the MBC header's dispatch leaves it */
      for (int j = 0; j < 3; j++) block(0, m + 12 * j, 12, 2); }
    return 0;
}
'''


def profiles(ref):
    text = open(os.path.join(ref, "tests", "protocol", "dmr", "test_dmr_dburst_profile.c")).read()
    body = text[text.index("static const expected_profile expected[]"):]
    body = body[:body.index("};")]
    rows = []
    for m in re.finditer(r"\{(0x[0-9A-F]+)U, (\d)U, (\d)U, (NULL|\"[^\"]*\"), (0x[0-9A-F]+|0)U, ([^,]+), (\d+)U, (\d+)U, (\d+)U\}", body):
        fl = m.group(6).strip()
        flags = [] if fl == "0U" else [t.strip() for t in fl.split("|")]
        rows.append(dict(databurst=int(m.group(1), 16), confirmed=int(m.group(2)), header_format=int(m.group(3)),
                         subtype=None if m.group(4) == "NULL" else m.group(4).strip('"'), crcmask=int(m.group(5), 16), flags=flags,
                         crclen=int(m.group(7)), pdu_len=int(m.group(8)), pdu_start=int(m.group(9))))
    assert len(rows) == 19, len(rows)
    return rows


def sequences(ref, oracle_ref):
    test = os.path.join(ref, "tests", "protocol", "dmr", "test_dmr_relaxed_header_ip.c")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "harness.c")
        open(src, "w").write(HARNESS % dict(test=test))
        exe = os.path.join(tmp, "harness")
        dmr = os.path.join(ref, "src", "protocol", "dmr")
        subprocess.check_call(["gcc", "-O1", "-w", "-DMBELIB_NO_HEADERS=1", "-I", os.path.join(ref, "include"), "-I", dmr,
                               "-I", os.path.join(ref, "tests", "test_support"), src, os.path.join(dmr, "dmr_block.c"), os.path.join(dmr, "dmr_ars.c"),
                               os.path.join(dmr, "dmr_block_crypto.c"), "-L", oracle_ref, "-ldsdneo_ref", "-Wl,-rpath," + oracle_ref,
                               "-Wl,--unresolved-symbols=ignore-all", "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def crc9_vectors(oracle_ref):
    lib = ctypes.CDLL(os.path.join(oracle_ref, "libdsdneo_ref.so"))
    lib.ComputeCrc9Bit.restype = ctypes.c_uint16
    lib.ComputeCrc9Bit.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    out = []
    for v in (dict(rate=7, dbsn=0x35, mask=0x0F0, payload=[(i * 5 + 3) & 1 for i in range(80)], flip=7),
              dict(rate=10, dbsn=0x12, mask=0x10F, payload=[((i ^ 0xA) + 1) & 1 for i in range(176)], flip=31),
              dict(rate=8, dbsn=0x5A, mask=0x1FF, payload=[(i * 7 + 1) & 1 for i in range(128)], flip=12)):
        span = np.array(v["payload"] + [(v["dbsn"] >> (6 - i)) & 1 for i in range(7)], np.uint8)
        v["crc9_ref"] = int(lib.ComputeCrc9Bit(span.ctypes.data, len(span)))
        out.append(v)
    return out


def main():
    ref, oracle_ref = sys.argv[1], sys.argv[2]
    out = dict(
        profiles=profiles(ref),
        sequences=sequences(ref, oracle_ref),
        crc9=crc9_vectors(oracle_ref),
        type1_bounds=dict(cap=3072, seed=dict(header_valid=1, block_counter=1, header_blocks=9, conf=0, header_format=7, sap=0),
                          cases=[dict(byte_ctr=0, block_len=12, want=12), dict(byte_ctr=3068, block_len=12, want=3072),
                                 dict(byte_ctr=60000, block_len=12, want=3072)] + [dict(byte_ctr=None, block_len=24, repeat=64, want_max=3072)]),
        type2_bounds=dict(seed=dict(header_valid=1, block_counter="blocks", header_format=0, crc_valid0=1), udt_blocks=[4, 127, 6, 7]))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dmr_pdu_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
