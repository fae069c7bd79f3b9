// ddn_bcode_dev.h - the small binary block codes of the device side: a code as a compile-time type (length, parity-check rows, how
// its syndrome table is filled, what it accepts), its syndrome -> positions-to-flip table as a compile-time constant, and the one
// decode the kernels run over it; beside them the perfect Golay(23,12) of the P25 and vocoder words as a 2048-entry syndrome ->
// error-pattern constant.  Everything is constexpr and compiles for the host as well (plain g++: tests/test_bcode_dev.py runs every
// code against the oracle and the reference on the CPU).  A table is a static member of a template, so a code object holds only the
// tables its kernels index.
//
// reference: src/fec/fec.c:133-838 - the syndrome by parity-check matrix, the correction positions by a table that the *_init() loops
// fill.  Those loops overwrite single slots of an entry, so for the distance-6 codes the survivor of colliding patterns depends on
// their order: the builders below keep it.
#ifndef DDN_BCODE_DEV_H
#define DDN_BCODE_DEV_H
#include <stdint.h>

#include "ddn_tables_fec3.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DDN_BCODE_HD     __host__ __device__ __forceinline__ constexpr
#define DDN_BCODE_CONST  __device__ const
#define DDN_BCODE_UNROLL _Pragma("unroll")
#else
#define DDN_BCODE_HD     inline constexpr
#define DDN_BCODE_CONST  const
#define DDN_BCODE_UNROLL
#endif

namespace ddn_bcode {

enum Family { HAMMING, GOLAY, QR, BARE }; // which builder fills the table, and the slots of an entry: 1, 3, 2; BARE: rows only
constexpr uint8_t NONE = 0xFF;            // an empty slot

// N bits (bit j of a word = rxBits[j]), K of them the message, R = N - K rows H: row i gives syndrome bit R - 1 - i.  A decode applies
// every position its entry names and then accepts when there are 1 .. ACCEPT of them.
template <int N, int K, const uint32_t (&ROWS)[N - K], Family F, int ACCEPT>
struct Code {
    static constexpr int n = N, k = K, r = N - K, accept = ACCEPT;
    static constexpr int slots = F == HAMMING ? 1 : F == GOLAY ? 3 : F == QR ? 2 : 0;
    static constexpr Family family = F;
    static constexpr const uint32_t (&H)[N - K] = ROWS;
};

// the P25 Hamming(10,6,3) (src/fec/hamming_10_6_3.cpp: word = data << 4 | check) and mbelib's Hamming(15,11) (ecc.c) state their own rows
constexpr uint32_t hamming_10_6_3_H[4] = {0x398u, 0x354u, 0x2E2u, 0x1E1u};
constexpr uint32_t mbe_hamming_15_11_H[4] = {0x7F08u, 0x78E4u, 0x66D2u, 0x55B1u};

// Hamming_*_decode (fec.c:145-170, 200-420): a syndrome that is no column of H refuses.  Hamming(15,11) is perfect and never does.
constexpr Code<7, 4, ddn_hamming_7_4_H, HAMMING, 1> HAMMING_7_4{};
constexpr Code<12, 8, ddn_hamming_12_8_H, HAMMING, 1> HAMMING_12_8{};
constexpr Code<13, 9, ddn_hamming_13_9_H, HAMMING, 1> HAMMING_13_9{};
constexpr Code<15, 11, ddn_hamming_15_11_H, HAMMING, 1> HAMMING_15_11{};
constexpr Code<16, 11, ddn_hamming_16_11_4_H, HAMMING, 1> HAMMING_16_11_4{};
// Golay_20_8_decode (fec.c:514-561) accepts up to two flips: the flips of a three-position entry are applied, then refused
constexpr Code<20, 8, ddn_golay_20_8_H, GOLAY, 2> GOLAY_20_8{};
// Golay_24_12_decode (fec.c:656-690) and QR_16_7_6_decode (fec.c:782-822) refuse only an empty entry
constexpr Code<24, 12, ddn_golay_24_12_H, GOLAY, 3> GOLAY_24_12{};
constexpr Code<16, 7, ddn_qr_16_7_6_H, QR, 2> QR_16_7_6{};
constexpr Code<10, 6, hamming_10_6_3_H, HAMMING, 1> HAMMING_10_6_3{}; // decoded by hamming_10_6_3_hard(), below
constexpr Code<15, 11, mbe_hamming_15_11_H, BARE, 1> MBE_HAMMING_15_11{};

template <class C>
DDN_BCODE_HD int
syndrome(C, uint32_t w) {
    int s = 0;
    DDN_BCODE_UNROLL
    for (int i = 0; i < C::r; i++) {
        s |= (__builtin_popcount(w & C::H[i]) & 1) << (C::r - 1 - i);
    }
    return s;
}

// a word from n bytes that hold one bit each
DDN_BCODE_HD uint32_t
pack_u8(const uint8_t* b, int n) {
    uint32_t w = 0;
    for (int j = 0; j < n; j++) {
        w |= (uint32_t)(b[j] & 1u) << j;
    }
    return w;
}

// ---- the tables ------------------------------------------------------------------------------------------------------------------------
template <class C>
struct Table {
    uint8_t t[1 << C::r][C::slots];
};

// correctable positions = the columns of H (the explicit assignments of Hamming_*_init(), fec.c:133-143,183-198,...)
template <class C>
constexpr void
build_hamming(C c, Table<C>& tab) {
    for (int p = 0; p < C::n; p++) {
        tab.t[syndrome(c, 1u << p)][0] = (uint8_t)p;
    }
}

// Golay_20_8_init / Golay_24_12_init (fec.c:437-512, 566-640): kd message bits, 12 parity bits, slot-wise assignments in the
// reference's loop order
template <class C>
constexpr void
build_golay(C c, Table<C>& tab) {
    constexpr int kd = C::k;
    auto& t = tab.t;
    auto S = [&](uint32_t w) { return syndrome(c, w); };
    auto P = [&](int ip) { return 1 << (11 - ip); };
    for (int i1 = 0; i1 < kd; i1++) {
        for (int i2 = i1 + 1; i2 < kd; i2++) {
            for (int i3 = i2 + 1; i3 < kd; i3++) {
                const int s = S((1u << i1) | (1u << i2) | (1u << i3));
                t[s][0] = (uint8_t)i1, t[s][1] = (uint8_t)i2, t[s][2] = (uint8_t)i3;
            }
            const int s = S((1u << i1) | (1u << i2));
            t[s][0] = (uint8_t)i1, t[s][1] = (uint8_t)i2;
            for (int ip = 0; ip < 12; ip++) {
                const int sp = s ^ P(ip);
                t[sp][0] = (uint8_t)i1, t[sp][1] = (uint8_t)i2, t[sp][2] = (uint8_t)(kd + ip);
            }
        }
        const int s = S(1u << i1);
        t[s][0] = (uint8_t)i1;
        for (int ip1 = 0; ip1 < 12; ip1++) {
            const int s1 = s ^ P(ip1);
            t[s1][0] = (uint8_t)i1, t[s1][1] = (uint8_t)(kd + ip1);
            for (int ip2 = ip1 + 1; ip2 < 12; ip2++) {
                const int s2 = s1 ^ P(ip2);
                t[s2][0] = (uint8_t)i1, t[s2][1] = (uint8_t)(kd + ip1), t[s2][2] = (uint8_t)(kd + ip2);
            }
        }
    }
    for (int ip1 = 0; ip1 < 12; ip1++) {
        const int s1 = P(ip1);
        t[s1][0] = (uint8_t)(kd + ip1);
        for (int ip2 = ip1 + 1; ip2 < 12; ip2++) {
            const int s2 = s1 ^ P(ip2);
            t[s2][0] = (uint8_t)(kd + ip1), t[s2][1] = (uint8_t)(kd + ip2);
            for (int ip3 = ip2 + 1; ip3 < 12; ip3++) {
                const int s3 = s2 ^ P(ip3);
                t[s3][0] = (uint8_t)(kd + ip1), t[s3][1] = (uint8_t)(kd + ip2), t[s3][2] = (uint8_t)(kd + ip3);
            }
        }
    }
}

// QR_16_7_6_init (fec.c:744-780): 7 message bits, 9 parity bits, up to two positions
template <class C>
constexpr void
build_qr(C c, Table<C>& tab) {
    auto& t = tab.t;
    auto S = [&](uint32_t w) { return syndrome(c, w); };
    auto P = [&](int ip) { return 1 << (8 - ip); };
    for (int i1 = 0; i1 < 7; i1++) {
        for (int i2 = i1 + 1; i2 < 7; i2++) {
            const int s = S((1u << i1) | (1u << i2));
            t[s][0] = (uint8_t)i1, t[s][1] = (uint8_t)i2;
        }
        const int s = S(1u << i1);
        t[s][0] = (uint8_t)i1;
        for (int ip = 0; ip < 9; ip++) {
            const int sp = s ^ P(ip);
            t[sp][0] = (uint8_t)i1, t[sp][1] = (uint8_t)(7 + ip);
        }
    }
    for (int ip1 = 0; ip1 < 9; ip1++) {
        const int s1 = P(ip1);
        t[s1][0] = (uint8_t)(7 + ip1);
        for (int ip2 = ip1 + 1; ip2 < 9; ip2++) {
            const int s2 = s1 ^ P(ip2);
            t[s2][0] = (uint8_t)(7 + ip1), t[s2][1] = (uint8_t)(7 + ip2);
        }
    }
}

template <class C>
constexpr Table<C>
build(C c) {
    static_assert(C::family != BARE, "a code without a table");
    static_assert(C::family == HAMMING || C::r == (C::family == GOLAY ? 12 : 9), "the parity positions of the init loops");
    Table<C> tab{};
    for (int s = 0; s < (1 << C::r); s++) {
        for (int q = 0; q < C::slots; q++) {
            tab.t[s][q] = NONE;
        }
    }
    if constexpr (C::family == HAMMING) {
        build_hamming(c, tab);
    } else if constexpr (C::family == GOLAY) {
        build_golay(c, tab);
    } else {
        build_qr(c, tab);
    }
    return tab;
}

// the table of code C, present in a code object (and in a host program) only where something indexes it
template <class C>
struct TableOf {
    static DDN_BCODE_CONST Table<C> v;
};
template <class C>
DDN_BCODE_CONST Table<C> TableOf<C>::v = build(C{});

// ---- decoding ---------------------------------------------------------------------------------------------------------------------------
// the *_decode() of the reference on a packed word: w corrected, true when accepted (see Code)
template <class C>
DDN_BCODE_HD bool
decode(C c, uint32_t& w) {
    const int s = syndrome(c, w);
    if (s == 0) {
        return true;
    }
    int q = 0;
    for (; q < C::slots; q++) {
        const uint8_t p = TableOf<C>::v.t[s][q];
        if (p == NONE) {
            break;
        }
        w ^= 1u << p;
    }
    return q != 0 && q <= C::accept;
}

// a Hamming code's verdict without the flip, for the callers that write back selectively: -1 for a code word, the position to flip,
// or NONE when the syndrome is no column
template <class C>
DDN_BCODE_HD int
position(C c, uint32_t w) {
    static_assert(C::family == HAMMING, "one position per entry");
    const int s = syndrome(c, w);
    return s == 0 ? -1 : (int)TableOf<C>::v.t[s][0];
}

// hamming_10_6_3_decode (src/fec/hamming_10_6_3.cpp:20-105) on word = data << 4 | check: 0 valid, 1 corrected (*fixed = the word with
// a data bit flipped; a wrong check bit is left), 2 uncorrectable.  Its sixteen positions sit in one register, a nibble each, 15 = NONE.
constexpr uint64_t hamming_10_6_3_nibbles = 0xF9847FF36FF2510Full;
DDN_BCODE_HD int
hamming_10_6_3_hard(uint32_t w, uint32_t* fixed) {
    const int syn = syndrome(HAMMING_10_6_3, w);
    *fixed = w;
    if (syn == 0) {
        return 0;
    }
    const uint32_t p = (uint32_t)((hamming_10_6_3_nibbles >> (4 * syn)) & 15u);
    if (p == 15u) {
        return 2;
    }
    if (p >= 4) {
        *fixed = w ^ (1u << p);
    }
    return 1;
}

// ---- the perfect Golay(23,12): syndrome -> the one error pattern of weight <= 3 (1 + 23 + 253 + 1771 = 2048) -------------------------
// Both users divide by the same generator, mirrored: the P25 words (Golay24.hpp) LSB first by 0xAE3, the remainder in the low eleven
// bits after twelve steps; the vocoder words (mbelib ecc.c) MSB first by 0xC75.
struct Golay23Lsb {
    static DDN_BCODE_HD uint32_t syndrome(uint32_t cw) {
        cw &= 0x7FFFFFu;
        DDN_BCODE_UNROLL
        for (int i = 0; i < 12; i++) {
            cw = (cw & 1u) ? ((cw ^ 0xAE3u) >> 1) : (cw >> 1);
        }
        return cw;
    }
};
struct Golay23Msb {
    static DDN_BCODE_HD uint32_t syndrome(uint32_t w) {
        DDN_BCODE_UNROLL
        for (int i = 22; i >= 11; i--) {
            if ((w >> i) & 1u) {
                w ^= 0xC75u << (i - 11);
            }
        }
        return w & 0x7FFu;
    }
};

struct Patterns23 {
    uint32_t e[2048];
};
template <class S>
constexpr Patterns23
build_golay23() {
    Patterns23 tab{};
    for (int a = 0; a < 23; a++) {
        for (int b = a; b < 23; b++) {
            for (int c = b; c < 23; c++) { // equal indices collapse to the lower weights
                const uint32_t e = (1u << a) | (1u << b) | (1u << c);
                tab.e[S::syndrome(e)] = e;
            }
        }
    }
    return tab;
}
template <class S>
struct Golay23 {
    static DDN_BCODE_CONST Patterns23 v;
};
template <class S>
DDN_BCODE_CONST Patterns23 Golay23<S>::v = build_golay23<S>();

// a wrong constant fails the build
namespace check {
constexpr bool
nibbles_are_the_columns() {
    const auto t = build(HAMMING_10_6_3);
    for (int s = 1; s < 16; s++) {
        if (((hamming_10_6_3_nibbles >> (4 * s)) & 15u) != (t.t[s][0] == NONE ? 15u : t.t[s][0])) {
            return false;
        }
    }
    return true;
}
static_assert(nibbles_are_the_columns(), "Hamming(10,6,3): the packed positions are the columns of its rows");
} // namespace check

} // namespace ddn_bcode
#endif
