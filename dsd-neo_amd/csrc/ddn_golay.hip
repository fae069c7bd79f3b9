// ddn_golay.hip — batched P25 Phase 1 Golay(24,12,8) / (18,6,8) decoders, hard and soft, and the soft Hamming(10,6,3).
//
//   k_golay24              == check_and_fix_golay_24_6 / check_and_fix_golay_24_12
//                             (src/protocol/p25/phase1/p25p1_check_hdu.cpp:28-37; include/dsd-neo/fec/Golay24.hpp:19-197,262-389)
//   k_golay24_soft         == check_and_fix_golay_24_{6,12}_soft   (src/protocol/p25/phase1/p25p1_soft.cpp:175-593)
//   k_hamming_10_6_3_soft  == hamming_10_6_3_soft                  (same file)
//
// One codeword per lane.  The [23,12,7] code is perfect, so the reference's systematic search always lands on the unique
// codeword within distance 3; here that is one lookup in a 2048-entry syndrome -> error-pattern table, and the reference's
// reported correction count is the pattern weight when the errors fit one cyclic window of 11 positions (its first pass) and
// one less otherwise (it had to flip a trial bit first).  On failure the data is left untouched.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ddn_bcode_dev.h"
#include "ddn_device.h"

namespace {
using Golay23 = ddn_bcode::Golay23<ddn_bcode::Golay23Lsb>; // the syndrome -> error pattern table
} // namespace

__global__ __launch_bounds__(256) void
k_golay24(uint8_t* __restrict__ data, const uint8_t* __restrict__ parity, int len, int n,
          uint8_t* __restrict__ status, int32_t* __restrict__ fixed, DdnSel sel) {
    const uint32_t* tab = Golay23::v.e; // (read in place - 8 KB, it stays in the L1: single-wave workgroups, no LDS; see DDN_WG)
    auto one = [&](long i) {
    uint8_t* d = data + (size_t)i * len;
    const uint8_t* p = parity + (size_t)i * 12;
    uint32_t cw = 0;
    bool valid = true;
    for (int k = 0; k < 12; k++) {
        const uint32_t v = p[k];
        valid &= v <= 1;
        cw |= (v & 1u) << (12 + k);
    }
    for (int k = 0; k < len; k++) {
        const uint32_t v = d[k];
        valid &= v <= 1;
        cw |= (v & 1u) << (12 - len + k);
    }
    int fx = 0, rc = 1;
    if (valid) {
        const uint32_t pbit = cw & 0x800000u;
        uint32_t w23 = cw & 0x7fffffu;
        const uint32_t e = tab[ddn_bcode::Golay23Lsb::syndrome(w23)];
        if (e) {
            const int wt = __popc(e);
            bool fits = false;
            uint32_t r = e;
#pragma unroll
            for (int k = 0; k < 23; k++) {
                fits |= (r & 0xFFFu) == 0;
                r = ((r << 1) | (r >> 22)) & 0x7fffffu;
            }
            fx = fits ? wt : wt - 1;
            w23 ^= e;
        }
        cw = w23 | pbit;
        const bool odd = (__popc(cw) & 1) != 0;
        if (!(odd && (cw & 0x3fu) != 0)) {
            rc = 0;
            for (int k = 0; k < len; k++) {
                d[k] = (uint8_t)((cw >> (12 - len + k)) & 1u);
            }
        }
    }
    status[i] = (uint8_t)rc;
    if (fixed) {
        fixed[i] = fx;
    }
    };
    ddn_sel_for_each(sel, (long)n, one);
}

// ---- soft (Chase) variants: src/protocol/p25/phase1/p25p1_soft.cpp:175-593 ------------------------------------------
// hamming_10_6_3_soft: seed with the hard decode, then flip every subset of <= 2 of the 5 least reliable bits and keep
// valid codewords; check_and_fix_golay_24_{6,12}_soft: seed with the hard decode, then every subset of <= 4 of the 8
// least reliable bits through the hard decoder.  Penalty = clamped reliability summed over the bits where the
// re-encoded codeword differs from the received word, ties to fewer differing bits, masks in increasing order with
// strict improvement only; a corrected hard decode wins unless the best candidate beats it by more than 8.
namespace {
__device__ __forceinline__ int
clamp255d(int v) {
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// returns 0 and the corrected 24-bit word, or 1 (odd overall parity with non-zero low six bits: DSDGolay24::decode_*)
__device__ __forceinline__ int
golay_hard_word(uint32_t cw, const uint32_t* tab, uint32_t* out, int* fx) {
    const uint32_t pbit = cw & 0x800000u;
    uint32_t w23 = cw & 0x7fffffu;
    const uint32_t e = tab[ddn_bcode::Golay23Lsb::syndrome(w23)];
    *fx = 0;
    if (e) {
        const int wt = __popc(e);
        bool fits = false;
        uint32_t r = e;
#pragma unroll
        for (int k = 0; k < 23; k++) {
            fits |= (r & 0xFFFu) == 0;
            r = ((r << 1) | (r >> 22)) & 0x7fffffu;
        }
        *fx = fits ? wt : wt - 1;
        w23 ^= e;
    }
    const uint32_t c2 = w23 | pbit;
    *out = c2;
    return ((__popc(c2) & 1) && (c2 & 0x3fu)) ? 1 : 0;
}

__device__ __forceinline__ uint32_t
golay_encode_word(uint32_t d12) {
    uint32_t cw = d12 & 0xFFFu;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        cw = (cw & 1u) ? ((cw ^ 0xAE3u) >> 1) : (cw >> 1);
    }
    uint32_t w = (cw << 12) | (d12 & 0xFFFu);
    if (__popc(w) & 1) {
        w ^= 0x800000u;
    }
    return w;
}
} // namespace

template <int L>
__global__ __launch_bounds__(256) void
k_golay24_soft(uint8_t* __restrict__ data, const uint8_t* __restrict__ parity, const int32_t* __restrict__ reliab, int n,
               uint8_t* __restrict__ status, int32_t* __restrict__ fixed) {
    constexpr int N = L + 12, SH = 12 - L;
    __shared__ uint32_t tab[2048];
    for (int i = threadIdx.x; i < 2048; i += 256) {
        tab[i] = Golay23::v.e[i];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    uint8_t* d = data + (size_t)i * L;
    const uint8_t* p = parity + (size_t)i * 12;
    const int32_t* rp = reliab + (size_t)i * N;
    uint32_t orig = 0;
    bool valid = true;
    int rel[N], key[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint32_t v = (k < L) ? d[k] : p[k - L];
        valid &= v <= 1;
        orig |= (v & 1u) << (k + SH);
        rel[k] = clamp255d(rp[k]);
        key[k] = rel[k] * 64 + k;
    }
    int rc = 1, fx_out = 0;
    if (valid) {
        const uint32_t nmask = ((1u << N) - 1u) << SH;
        auto penalty = [&](uint32_t diff, int* nd) {
            int pen = 0;
#pragma unroll
            for (int k = 0; k < N; k++) {
                pen += ((diff >> (k + SH)) & 1u) ? rel[k] : 0;
            }
            *nd = __popc(diff);
            return pen;
        };
        int best_pen = 999999, best_fixed = 0, hard_pen = 999999, hard_fixed = 0;
        bool found = false, hard_valid = false, hard_corr = false;
        uint32_t best_dw = 0, hard_dw = 0;
        {
            uint32_t c2;
            if (golay_hard_word(orig, tab, &c2, &hard_fixed) == 0) {
                hard_dw = c2 & (0xFFFu & ~((1u << SH) - 1u));
                int nd;
                hard_pen = penalty((orig ^ golay_encode_word(hard_dw)) & nmask, &nd);
                best_pen = hard_pen;
                best_fixed = nd;
                best_dw = hard_dw;
                hard_valid = true;
                hard_corr = hard_fixed > 0;
                found = true;
            }
        }
        // the 8 least reliable positions in (reliability, position) order -> the word bits they flip
        uint32_t flip[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            int bk = key[0], bi = 0;
#pragma unroll
            for (int k = 1; k < N; k++) {
                const bool lt = key[k] < bk;
                bk = lt ? key[k] : bk;
                bi = lt ? k : bi;
            }
#pragma unroll
            for (int k = 0; k < N; k++) {
                key[k] = (k == bi) ? 0x7fffffff : key[k];
            }
            flip[j] = 1u << (bi + SH);
        }
        for (int mask = 0; mask < 256; mask++) {
            if (__popc((unsigned)mask) > 4) {
                continue;
            }
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                x ^= (mask & (1 << b)) ? flip[b] : 0u;
            }
            uint32_t c2;
            int cf;
            if (golay_hard_word(orig ^ x, tab, &c2, &cf) != 0) {
                continue;
            }
            const uint32_t dw = c2 & (0xFFFu & ~((1u << SH) - 1u));
            int nd;
            const int pen = penalty((orig ^ golay_encode_word(dw)) & nmask, &nd);
            if (pen < best_pen || (pen == best_pen && nd < best_fixed)) {
                best_pen = pen;
                best_fixed = nd;
                best_dw = dw;
                found = true;
            }
        }
        if (found) {
            rc = 0;
            uint32_t out_dw = best_dw;
            fx_out = best_fixed;
            if (hard_valid && hard_corr && best_dw != hard_dw && best_pen + 8 >= hard_pen) {
                out_dw = hard_dw;
                fx_out = hard_fixed;
            }
#pragma unroll
            for (int k = 0; k < L; k++) {
                d[k] = (uint8_t)((out_dw >> (k + SH)) & 1u);
            }
        }
    }
    status[i] = (uint8_t)rc;
    if (fixed) {
        fixed[i] = fx_out;
    }
}

__global__ __launch_bounds__(256) void
k_hamming_10_6_3_soft(const uint8_t* __restrict__ bits, const int32_t* __restrict__ reliab, int n,
                      uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint8_t* b = bits + (size_t)i * 10;
    const int32_t* rp = reliab + (size_t)i * 10;
    int rel[10], key[10];
    uint32_t orig = 0; // bit (9 - k) = element k: (data << 4) | check, data[0] the MSB
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 10; k++) {
        const uint32_t v = b[k];
        valid &= v <= 1;
        orig |= (v & 1u) << (9 - k);
        rel[k] = clamp255d(rp[k]);
        key[k] = rel[k] * 64 + k;
    }
    auto encode = [&](uint32_t w) -> uint32_t {
        const uint32_t d0 = (w >> 9) & 1, d1 = (w >> 8) & 1, d2 = (w >> 7) & 1, d3 = (w >> 6) & 1, d4 = (w >> 5) & 1,
                       d5 = (w >> 4) & 1;
        const uint32_t p0 = d0 ^ d1 ^ d2 ^ d5, p1 = d0 ^ d1 ^ d3 ^ d5, p2 = d0 ^ d2 ^ d3 ^ d4, p3 = d1 ^ d2 ^ d3 ^ d4;
        return (w & 0x3F0u) | (p0 << 3) | (p1 << 2) | (p2 << 1) | p3;
    };
    auto penalty = [&](uint32_t diff) {
        int pen = 0;
#pragma unroll
        for (int k = 0; k < 10; k++) {
            pen += ((diff >> (9 - k)) & 1u) ? rel[k] : 0;
        }
        return pen;
    };
    int rc = 2;
    uint32_t outw = orig;
    if (valid) {
        int best_pen = 999999, best_flips = 99, hard_pen = 999999;
        bool found = false, hard_valid = false, hard_corr = false;
        uint32_t best = 0, hardw = 0;
        {
            uint32_t fw;
            const int r = ddn_bcode::hamming_10_6_3_hard(orig, &fw);
            if (r == 0 || r == 1) {
                hardw = encode(fw);
                hard_valid = true;
                hard_corr = (r == 1);
                hard_pen = penalty(orig ^ hardw);
                best_pen = hard_pen;
                best_flips = __popc(orig ^ hardw);
                best = hardw;
                found = true;
            }
        }
        uint32_t flip[5];
#pragma unroll
        for (int j = 0; j < 5; j++) {
            int bk = key[0], bi = 0;
#pragma unroll
            for (int k = 1; k < 10; k++) {
                const bool lt = key[k] < bk;
                bk = lt ? key[k] : bk;
                bi = lt ? k : bi;
            }
#pragma unroll
            for (int k = 0; k < 10; k++) {
                key[k] = (k == bi) ? 0x7fffffff : key[k];
            }
            flip[j] = 1u << (9 - bi);
        }
        for (int mask = 0; mask < 32; mask++) {
            const int nf = __popc((unsigned)mask);
            if (nf > 2) {
                continue;
            }
            uint32_t x = 0;
#pragma unroll
            for (int q = 0; q < 5; q++) {
                x ^= (mask & (1 << q)) ? flip[q] : 0u;
            }
            uint32_t fw;
            if (ddn_bcode::hamming_10_6_3_hard(orig ^ x, &fw) != 0) {
                continue;
            }
            const uint32_t c = orig ^ x;
            const int pen = penalty(orig ^ c);
            if (pen < best_pen || (pen == best_pen && nf < best_flips)) {
                best_pen = pen;
                best_flips = nf;
                best = c;
                found = true;
            }
        }
        if (found) {
            if (hard_valid && hard_corr && best != hardw && best_pen + 8 >= hard_pen) {
                outw = hardw;
                rc = 1;
            } else {
                outw = best;
                rc = (best == orig) ? 0 : 1;
            }
        }
    }
    uint8_t* o = out + (size_t)i * 10;
    if (valid) {
#pragma unroll
        for (int k = 0; k < 10; k++) {
            o[k] = (uint8_t)((outw >> (9 - k)) & 1u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 10; k++) {
            o[k] = b[k];
        }
    }
    status[i] = (uint8_t)rc;
}

extern "C" hipError_t
ddn_dev_golay24_soft(uint8_t* data, const uint8_t* parity, const int32_t* reliab, int len, int n, uint8_t* status,
                     int32_t* fixed, hipStream_t st) {
    if (n <= 0) {
        return hipSuccess;
    }
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    if (len == 6) {
        hipLaunchKernelGGL((k_golay24_soft<6>), grid, blk, 0, st, data, parity, reliab, n, status, fixed);
    } else {
        hipLaunchKernelGGL((k_golay24_soft<12>), grid, blk, 0, st, data, parity, reliab, n, status, fixed);
    }
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_hamming_10_6_3_soft(const uint8_t* bits, const int32_t* reliab, int n, uint8_t* out, uint8_t* status,
                            hipStream_t st) {
    if (n <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_hamming_10_6_3_soft, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bits, reliab, n, out,
                       status);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_golay24(uint8_t* data, const uint8_t* parity, int len, int n, uint8_t* status, int32_t* fixed, hipStream_t st) {
    if (n <= 0) {
        return hipSuccess;
    }
    const DdnSel sel = ddn_sel_for(len == 6 ? 36 : 12);
    hipLaunchKernelGGL(k_golay24, dim3(ddn_sel_grid(&sel, ((unsigned long)n + DDN_WG - 1) / DDN_WG)), dim3(DDN_WG), 0, st, data, parity, len, n,
                       status, fixed, sel);
    return hipGetLastError();
}
