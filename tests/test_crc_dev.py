"""dsd-neo_amd/csrc/ddn_crc_dev.h compiled for the host (g++ -std=c++17, no GPU): every named code over seeded random messages of
every length from 1 to 400 bits - which covers what the kernels feed them: 26, 41, 48, 80, 135, 144, 164, 168, 176, 224 - against
the compiled reference where it has the function (oracle/_ref), the CPU oracle's own restatements, and the Python restatements the
protocol tests use; and the header's table, column and span-folding forms against its bit-serial form."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dpmr
import dstar
import orc
import p25gen
import rx4

needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="compiled reference (oracle/_ref) not present")

CODES = ["CCITT16", "CRC9", "CRC32", "M17", "P25_CRC12", "NXDN_CRC6", "NXDN_CRC12F", "DPMR_CRC7", "DSTAR_X25"]
WIDTH = dict(CCITT16=16, CRC9=9, CRC32=32, M17=16, P25_CRC12=12, NXDN_CRC6=6, NXDN_CRC12F=12, DPMR_CRC7=7, DSTAR_X25=16)
MAX_BITS = 400

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ddn_crc_dev.h"
using namespace ddn_crc;
static const Code codes[9] = {CCITT16, CRC9, CRC32, M17, P25_CRC12, NXDN_CRC6, NXDN_CRC12F, DPMR_CRC7, DSTAR_X25};
static uint32_t rnd_state = 0x2545F491u;
static uint32_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 17; rnd_state ^= rnd_state << 5; return rnd_state; }

// wave_crc()'s folding with the 64 lanes in an array: lane i reads lane i + s where the wavefront shuffles down by s
static uint32_t fold64(const Code c, const std::vector<uint8_t>& msg) {
    const int n = (int)msg.size();
    uint32_t v[64 + 64] = {0};
    for (int lane = 0; lane < 64; lane++) {
        v[lane] = span_crc(c, n, lane, [&](int j) { return (uint32_t)msg[j]; });
    }
    uint32_t m = span_shift(c, n);
    for (int s = 1; s < 64; s <<= 1) {
        uint32_t nv[64];
        for (int lane = 0; lane < 64; lane++) {
            const uint32_t right = lane + s < 64 ? v[lane + s] : v[lane]; // (__shfl_down past the end returns the lane's own)
            nv[lane] = (lane & (2 * s - 1)) == 0 ? (gf2_mulmod(c, v[lane], m) ^ right) : v[lane];
        }
        for (int lane = 0; lane < 64; lane++) {
            v[lane] = nv[lane];
        }
        m = gf2_mulmod(c, m, m);
    }
    return v[0];
}

int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb"); // per message: its bits, one per byte, MAX_BITS of them; message k has k + 1 bits
    const int max_bits = atoi(argv[2]);
    std::vector<uint8_t> all((size_t)max_bits * max_bits);
    if (!f || fread(all.data(), 1, all.size(), f) != all.size()) {
        return 2;
    }
    fclose(f);
    unsigned long long bad = 0;
    for (int k = 0; k < max_bits; k++) {
        const int n = k + 1;
        const uint8_t* b = all.data() + (size_t)k * max_bits;
        printf("%d", n);
        for (int ci = 0; ci < 9; ci++) {
            const Code c = codes[ci];
            const uint32_t serial = of_bits_u8(c, n, b);
            printf(" %u", serial);
            bad += of_bits(c, n, [&](int i) { return b[i] & 1u; }) != serial; // a callable
            uint32_t reg = c.init; // a bit at a time
            for (int i = 0; i < n; i++) {
                reg = bit(c, reg, b[i]);
            }
            bad += finish(c, reg) != serial;
            uint32_t tail = 0; // the last `width` bits read as a check field
            for (int i = n < c.width ? n : n - c.width; i < n; i++) {
                tail = tail * 2u + b[i];
            }
            bad += n >= c.width && field_u8(b + n - c.width, c.width) != tail;
            if (c.init == 0) { // the columns: the register is the XOR of the set bits' contributions
                uint32_t x = 0;
                for (int i = 0; i < n; i++) {
                    x ^= b[i] ? column(c, n, i) : 0u;
                }
                bad += finish(c, x) != serial;
            }
            if (n % 8 == 0) { // packed bytes, in the code's bit order; the table; the span folding
                std::vector<uint8_t> by(n / 8);
                for (int i = 0; i < n; i++) {
                    by[i >> 3] |= (uint8_t)(b[i] << (c.reflected ? (i & 7) : 7 - (i & 7)));
                }
                bad += of_bytes(c, by.data(), n / 8) != serial;
                if (!c.reflected && c.width >= 8) {
                    const ByteTable t = byte_table(c);
                    uint32_t r = c.init;
                    for (int i = 0; i < n / 8; i++) {
                        r = byte(c, t, r, by[i]);
                    }
                    bad += finish(c, r) != serial;
                }
                if (!c.reflected && c.init == 0) {
                    bad += finish(c, fold64(c, by)) != serial;
                }
            }
        }
        printf("\n");
    }
    const int lens[5] = {1, 63, 64, 65, 3072}; // bytes: one span lane, a lane short of / exactly / a lane over one byte each, a full DMR row
    for (int li = 0; li < 5; li++) {
        std::vector<uint8_t> msg(lens[li]);
        for (auto& x : msg) {
            x = (uint8_t)(rnd() >> 24);
        }
        bad += fold64(CCITT16, msg) != bytes(CCITT16, 0u, msg.data(), lens[li]);
        bad += fold64(CRC32, msg) != bytes(CRC32, 0u, msg.data(), lens[li]);
    }
    printf("bad %llu\n", bad);
    return 0;
}
'''


def _bits_of(v, width):
    return [(v >> (width - 1 - i)) & 1 for i in range(width)]


@pytest.fixture(scope="module")
def run():
    """-> (messages [400][400] one bit per byte, message k = the first k + 1 of row k; {code: [400] checksums}; forms that disagreed)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(20251)
    msgs = rng.integers(0, 2, (MAX_BITS, MAX_BITS), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        msgs.tofile(os.path.join(d, "msgs.bin"))
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(root, "dsd-neo_amd", "csrc"), os.path.join(d, "t.cpp"), "-o", exe])
        lines = subprocess.check_output([exe, os.path.join(d, "msgs.bin"), str(MAX_BITS)]).decode().splitlines()
    assert len(lines) == MAX_BITS + 1
    vals = np.array([[int(x) for x in ln.split()] for ln in lines[:-1]], np.int64)
    assert list(vals[:, 0]) == list(range(1, MAX_BITS + 1))
    return msgs, {c: vals[:, 1 + i] for i, c in enumerate(CODES)}, int(lines[-1].split()[1])


def _msg(msgs, n):
    return np.ascontiguousarray(msgs[n - 1, :n])


def test_table_column_and_span_forms_equal_the_serial_form(run):
    """per bit, per callable, per packed byte, the byte table, the XOR of per-bit columns and wave_crc()'s span folding (the shuffle
    replaced by an array; also at 1, 63, 64, 65 and 3072 bytes) all give the one-bit-per-byte form's value, for every code they apply to;
    field_u8() reads a check field first bit most significant"""
    assert run[2] == 0


def test_m17_check_value(run):
    """the M17 specification's check value, and the CRC-16/X25 one D-STAR's code is catalogued under"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "c.cpp")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "ddn_crc_dev.h"\nint main() { const uint8_t* s = (const uint8_t*)"123456789";\n'
                    'printf("%u %u\\n", ddn_crc::of_bytes(ddn_crc::M17, s, 9), ddn_crc::of_bytes(ddn_crc::DSTAR_X25, s, 9)); }\n')
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(root, "dsd-neo_amd", "csrc"), src, "-o", os.path.join(d, "c")])
        m17v, x25 = subprocess.check_output([os.path.join(d, "c")]).split()
    assert int(m17v) == 0x772B and int(x25) == 0x906E


def test_against_the_oracle(run):
    """orc_ysf_crc16 (the division over message + field leaves 0 behind its complement), orc_m17_crc16 and orc_p25_crc16_ok, each also
    with one flipped message bit and one flipped field bit"""
    msgs, got, _ = run
    o = orc.oracle()
    o.orc_ysf_crc16.restype = C.c_uint16
    o.orc_ysf_crc16.argtypes = [C.c_void_p, C.c_int]
    o.orc_m17_crc16.restype = C.c_uint16
    o.orc_m17_crc16.argtypes = [C.c_void_p, C.c_int]
    o.orc_p25_crc16_ok.argtypes = [C.c_void_p, C.c_int]
    for n in range(1, MAX_BITS + 1):
        m = _msg(msgs, n)
        frame = np.concatenate([m, np.array(_bits_of(int(got["CCITT16"][n - 1]), 16), np.uint8)])
        assert o.orc_ysf_crc16(frame.ctypes.data, n + 16) == 0, n
        for flip in (n // 2, n + 5):
            bad = frame.copy()
            bad[flip] ^= 1
            assert o.orc_ysf_crc16(bad.ctypes.data, n + 16) != 0, (n, flip)
        if n % 8 == 0:
            by = np.packbits(m)
            assert int(got["M17"][n - 1]) == o.orc_m17_crc16(by.ctypes.data, n // 8), n
            fr = np.packbits(frame)
            assert o.orc_p25_crc16_ok(fr.ctypes.data, n // 8) == 0, n
            for flip in (n // 2, n + 5):
                bad = fr.copy()
                bad[flip >> 3] ^= 0x80 >> (flip & 7)
                assert o.orc_p25_crc16_ok(bad.ctypes.data, n // 8) != 0, (n, flip)


def test_against_the_python_restatements(run):
    """D-STAR (tests/dstar.py, whole octets, LSB first, byte-swapped), dPMR (tests/dpmr.py) and NXDN (tests/rx4.py: 26 + 6 and 80 + 12
    bits, good and with a flipped message / field bit); CRC9 and CRC32 against the generators' (tests/p25gen.py)"""
    msgs, got, _ = run
    for n in range(1, MAX_BITS + 1):
        m = _msg(msgs, n)
        assert int(got["DPMR_CRC7"][n - 1]) == dpmr.crc7(m), n
        assert int(got["CRC9"][n - 1]) == p25gen.crc9(m), n
        if n % 8 == 0:
            v = int(got["DSTAR_X25"][n - 1])
            assert (((v & 0xFF) << 8) | (v >> 8)) == dstar.crc16(np.packbits(m, bitorder="little")), n
            assert int(got["CRC32"][n - 1]) == p25gen.crc32mbf(np.packbits(m), n), n
    for kind, (n, code) in enumerate(((26, "NXDN_CRC6"), (80, "NXDN_CRC12F"))):
        frame = np.concatenate([_msg(msgs, n), np.array(_bits_of(int(got[code][n - 1]), WIDTH[code]), np.uint8)])
        assert rx4.nxdn_crc_ok(frame, kind)
        for flip in (3, n + 2):
            bad = frame.copy()
            bad[flip] ^= 1
            assert not rx4.nxdn_crc_ok(bad, kind)


@needs_ref
def test_against_the_compiled_reference(run):
    """ComputeCrcCCITT16b and ComputeCrcCCITT (80 bits), crc16_lb_bridge and crc12_xb_bridge (message + field -> 0, a flipped bit ->
    not 0; their buffers hold 190 bits), ComputeCrc9Bit, ComputeCrc32Bit (the register without the inversion, its bytes reversed),
    m17_crc16"""
    msgs, got, _ = run
    r = orc.ref()
    r.ComputeCrcCCITT16b.restype = C.c_uint16
    r.ComputeCrcCCITT16b.argtypes = [C.c_void_p, C.c_uint]
    r.ComputeCrcCCITT.restype = C.c_uint16
    r.ComputeCrcCCITT.argtypes = [C.c_void_p]
    r.ComputeCrc9Bit.restype = C.c_uint16
    r.ComputeCrc9Bit.argtypes = [C.c_void_p, C.c_uint32]
    r.ComputeCrc32Bit.restype = C.c_uint32
    r.ComputeCrc32Bit.argtypes = [C.c_void_p, C.c_uint32]
    r.m17_crc16.restype = C.c_uint16
    r.m17_crc16.argtypes = [C.c_void_p, C.c_uint16]
    r.crc16_lb_bridge.argtypes = [C.c_void_p, C.c_int]
    r.crc12_xb_bridge.argtypes = [C.c_void_p, C.c_int]
    for n in range(1, MAX_BITS + 1):
        m = _msg(msgs, n)
        assert int(got["CCITT16"][n - 1]) == r.ComputeCrcCCITT16b(m.ctypes.data, n), n
        assert int(got["CRC9"][n - 1]) == r.ComputeCrc9Bit(m.ctypes.data, n), n
        raw = int(got["CRC32"][n - 1]) ^ 0xFFFFFFFF
        assert int.from_bytes(raw.to_bytes(4, "big"), "little") == r.ComputeCrc32Bit(m.ctypes.data, n), n
        if n == 80:
            assert int(got["CCITT16"][n - 1]) == r.ComputeCrcCCITT(m.ctypes.data)
        if n % 8 == 0:
            by = np.packbits(m)
            assert int(got["M17"][n - 1]) == r.m17_crc16(by.ctypes.data, n // 8), n
        for code, fn, w in (("CCITT16", r.crc16_lb_bridge, 16), ("P25_CRC12", r.crc12_xb_bridge, 12)):
            if n + w > 190:
                continue
            frame = np.concatenate([m, np.array(_bits_of(int(got[code][n - 1]), w), np.uint8)]).astype(np.int32)
            assert fn(frame.ctypes.data, n) == 0, (code, n)
            for flip in (n // 2, n + 3):
                bad = frame.copy()
                bad[flip] ^= 1
                assert fn(bad.ctypes.data, n) != 0, (code, n, flip)
