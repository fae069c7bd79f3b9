// ddn_crc_dev.h - every frame checksum of the device side: a CRC as a compile-time description, one register step, and the forms
// the kernels run over it (a bit, a byte, n bits, n packed bytes; a byte table, per-bit columns and span-per-lane folding for the
// three places that do not go bit by bit).  Everything but the wavefront shuffle is constexpr and compiles for the host as well
// (plain g++: tests/test_crc_dev.py runs every code against the reference and the oracle on the CPU).
#ifndef DDN_CRC_DEV_H
#define DDN_CRC_DEV_H
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DDN_CRC_HD     __host__ __device__ __forceinline__ constexpr
#define DDN_CRC_UNROLL _Pragma("unroll")
#else
#define DDN_CRC_HD inline constexpr
#define DDN_CRC_UNROLL
#endif

namespace ddn_crc {

struct Code {
    int width;       // register bits, 1 .. 32
    uint32_t poly;   // the generator below its leading term (bit-reversed when `reflected`)
    uint32_t init;   // register before the first bit
    uint32_t xorout; // added to the register after the last one
    bool reflected;  // false: bits enter at the register's top, a byte most significant bit first; true: at its bottom, LSB first
};

// CRC-CCITT, x^16 + x^12 + x^5 + 1, zero start, inverted: ComputeCrcCCITT16b() / crc16_lb_bridge() (src/protocol/p25/p25_crc.c:17-75),
// ComputeCrcCCITT() (dmr_utils.c:253-275), and ysf_crc16() (ysf.c:229-242), whose division over message + field leaves
// crc(message) ^ field = 0xFFFF on a good frame
constexpr Code CCITT16{16, 0x1021u, 0u, 0xFFFFu, false};
// x^9 + x^6 + x^4 + x^3 + 1, inverted: ComputeCrc9Bit() (dmr_utils.c:410-435) of the confirmed data blocks, DMR and P25
constexpr Code CRC9{9, 0x059u, 0u, 0x1FFu, false};
// crc32mbf() (src/protocol/p25/p25_crc.c:47-60) and ComputeCrc32Bit() of the DMR assembler: the second does not invert
constexpr Code CRC32{32, 0x04C11DB7u, 0u, 0xFFFFFFFFu, false};
// m17_crc16() (src/protocol/m17/m17_algorithms.c:19-35)
constexpr Code M17{16, 0x5935u, 0xFFFFu, 0u, false};
// x^12 + x^11 + x^7 + x^4 + x^2 + x + 1 (0x1897 with its leading term), remainder inverted: crc12_xb_bridge() (p25_crc.c:78-147)
constexpr Code P25_CRC12{12, 0x897u, 0u, 0xFFFu, false};
// x^6 + x^5 + x^2 + x + 1 (nxdn_deperm.c:1246-1261) and x^12 + x^11 + x^3 + x^2 + x + 1 (crc12f, nxdn_dcr_utils.c:21-42)
constexpr Code NXDN_CRC6{6, 0x27u, 0x3Fu, 0u, false};
constexpr Code NXDN_CRC12F{12, 0x80Fu, 0xFFFu, 0u, false};
// x^15 + x^14 + x^11 + x^10 + x^7 + x^6 + x^2 + 1: crc15() of FACCH2 / UDCH (nxdn_dcr_utils.c:44-69)
constexpr Code NXDN_CRC15{15, 0x4CC5u, 0x7FFFu, 0u, false};
// crc16cac() (nxdn_deperm.c:1263-1275) divides message + field by x^16 + x^12 + x^5 + 1 from a register of 0xC3EE and inverts: as
// with ysf_crc16() the division leaves crc(message) ^ field, so a good CAC (remainder 0) carries crc(message) in its field.  The
// division's register runs sixteen bits ahead of this form's: the start value is 0xC3EE shifted through sixteen zeros (check, below)
constexpr Code NXDN_CRC16CAC{16, 0x1021u, 0x5FE7u, 0xFFFFu, false};
// x^7 + x^3 + 1: dpmr_crc7()
constexpr Code DPMR_CRC7{7, 0x09u, 0u, 0u, false};
// CRC-16/X25: dstar_crc16() (dstar_header_utils.c), which returns it byte-swapped - the frame carries the low byte first
constexpr Code DSTAR_X25{16, 0x8408u, 0xFFFFu, 0xFFFFu, true};

DDN_CRC_HD uint32_t
mask(const Code c) {
    return 0xFFFFFFFFu >> (32 - c.width);
}

// the register after one more message bit (0 or 1)
DDN_CRC_HD uint32_t
bit(const Code c, uint32_t reg, uint32_t b) {
    if (c.reflected) {
        return ((reg ^ b) & 1u) ? ((reg >> 1) ^ c.poly) : (reg >> 1);
    }
    return (((reg >> (c.width - 1)) & 1u) ^ b) ? (((reg << 1) ^ c.poly) & mask(c)) : ((reg << 1) & mask(c));
}

DDN_CRC_HD uint32_t
byte(const Code c, uint32_t reg, uint32_t v) {
    DDN_CRC_UNROLL
    for (int j = 7; j >= 0; j--) {
        reg = bit(c, reg, (v >> (c.reflected ? 7 - j : j)) & 1u);
    }
    return reg;
}

// n bits get(0) .. get(n - 1), each 0 or 1
template <class Get>
DDN_CRC_HD uint32_t
bits(const Code c, uint32_t reg, int n, Get get) {
    for (int i = 0; i < n; i++) {
        reg = bit(c, reg, (uint32_t)get(i));
    }
    return reg;
}
// ... of an array that holds one bit per byte
DDN_CRC_HD uint32_t
bits_u8(const Code c, uint32_t reg, int n, const uint8_t* p) {
    for (int i = 0; i < n; i++) {
        reg = bit(c, reg, p[i] & 1u);
    }
    return reg;
}

DDN_CRC_HD uint32_t
bytes(const Code c, uint32_t reg, const uint8_t* p, int n) {
    for (int i = 0; i < n; i++) {
        reg = byte(c, reg, p[i]);
    }
    return reg;
}

DDN_CRC_HD uint32_t
finish(const Code c, uint32_t reg) {
    return reg ^ c.xorout;
}

// the whole checksum, as the frame carries it
DDN_CRC_HD uint32_t
of_bytes(const Code c, const uint8_t* p, int n) {
    return finish(c, bytes(c, c.init, p, n));
}
template <class Get>
DDN_CRC_HD uint32_t
of_bits(const Code c, int n, Get get) {
    return finish(c, bits(c, c.init, n, get));
}
DDN_CRC_HD uint32_t
of_bits_u8(const Code c, int n, const uint8_t* p) {
    return finish(c, bits_u8(c, c.init, n, p));
}
// a received check field held one bit per byte, first bit most significant
DDN_CRC_HD uint32_t
field_u8(const uint8_t* p, int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; i++) {
        v = (v << 1) | (p[i] & 1u);
    }
    return v;
}

// ---- a byte at a time through a table (codes that enter at the top, 8 bits or wider) ---------------------------------------------
struct ByteTable {
    uint32_t t[256];
};
DDN_CRC_HD ByteTable
byte_table(const Code c) {
    ByteTable r{};
    for (uint32_t i = 0; i < 256; i++) {
        r.t[i] = byte(c, 0u, i);
    }
    return r;
}
DDN_CRC_HD uint32_t
byte(const Code c, const ByteTable& tab, uint32_t reg, uint32_t v) {
    return ((reg << 8) & mask(c)) ^ tab.t[((reg >> (c.width - 8)) ^ v) & 0xFFu];
}

// ---- a register that starts at zero is linear in the message -----------------------------------------------------------------------
// what message bit i of n puts into the final register: a lone one shifted through the remaining bits.  The register of a message
// is the XOR of its set bits' columns.
DDN_CRC_HD uint32_t
column(const Code c, int n, int i) {
    uint32_t reg = 0;
    for (int k = 0; k < n; k++) {
        reg = bit(c, reg, (k == i) ? 1u : 0u);
    }
    return reg;
}

// a * b mod the generator, both of degree < width
DDN_CRC_HD uint32_t
gf2_mulmod(const Code c, uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = c.width - 1; i >= 0; i--) {
        r = bit(c, r, 0u);
        r ^= ((b >> i) & 1u) ? a : 0u;
    }
    return r;
}

// The register (zero start) over n bytes get(0) .. get(n - 1) on 64 lanes.  Such a register is blind to leading zeros, so the message
// is right-aligned on 64 spans of `per` bytes: every lane runs its span from 0 (span_crc), and a tree folds them - the left half of
// a pair times x^(8 * per * width of the right half) (span_shift, squared at every level), plus the right half.
template <class Get>
DDN_CRC_HD uint32_t
span_crc(const Code c, int n, int lane, Get get) {
    const int per = (n + 63) / 64;
    const int first = n - (64 - lane) * per;
    uint32_t v = 0;
    for (int i = 0; i < per; i++) {
        const int j = first + i;
        if (j >= 0) {
            v = byte(c, v, get(j));
        }
    }
    return v;
}
DDN_CRC_HD uint32_t
span_shift(const Code c, int n) { // x^(8 * per)
    uint32_t m = 1;
    for (int i = 0; i < (n + 63) / 64; i++) {
        m = byte(c, m, 0u);
    }
    return m;
}
#ifdef __HIPCC__
template <class Get>
__device__ __forceinline__ uint32_t
wave_crc(const Code c, int n, int lane, Get get) { // every lane returns the total
    uint32_t v = span_crc(c, n, lane, get);
    uint32_t m = span_shift(c, n);
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t right = (uint32_t)__shfl_down((int)v, s, 64);
        if ((lane & (2 * s - 1)) == 0) {
            v = gf2_mulmod(c, v, m) ^ right;
        }
        m = gf2_mulmod(c, m, m);
    }
    return (uint32_t)__shfl((int)v, 0, 64);
}
#endif

// a wrong constant fails the build: the catalogued check values over "123456789" (M17's is its specification's)
namespace check {
constexpr uint8_t digits[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
static_assert(of_bytes(M17, digits, 9) == 0x772Bu, "M17");
static_assert(of_bytes(DSTAR_X25, digits, 9) == 0x906Eu, "CRC-16/X25");
static_assert(of_bytes(CCITT16, digits, 9) == (0x31C3u ^ 0xFFFFu), "CRC-16/XMODEM, inverted");
static_assert(of_bytes(CRC32, digits, 9) == 0x765E7680u, "CRC-32/CKSUM");
static_assert(byte(CRC32, byte_table(CRC32), 0x12345678u, 0x9Au) == byte(CRC32, 0x12345678u, 0x9Au), "table form");
static_assert(byte(NXDN_CRC16CAC, byte(NXDN_CRC16CAC, 0xC3EEu, 0u), 0u) == NXDN_CRC16CAC.init, "crc16cac's register, sixteen bits on");
} // namespace check

} // namespace ddn_crc
#endif
