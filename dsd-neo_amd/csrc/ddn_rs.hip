// ddn_rs.hip — batched Reed-Solomon decoders over GF(64) (ddn_gf64_dev.h), one codeword per lane.
//
//   k_rs63       == check_and_fix_reedsolomon_24_12_13 / _24_16_9 / check_and_fix_redsolomon_36_20_17
//                   (p25p1_check_ldu.cpp, p25p1_check_hdu.cpp:39-46; include/dsd-neo/fec/ReedSolomon.hpp:334-582,738-772,
//                   adapters :836-866,933-963,1028-1058)
//   k_rs63_soft  == p25p1_rs_24_12_13_soft_reliability / _24_16_9_ / _36_20_17_ (see the kernel)
//   k_rs28_*     == ez_rs28_ess / _facch / _sacch over the vendored ezpwd RS<63,35> (see "P25 Phase 2 RS(63,35)" below)
//
// The two Phase 1 kernels share one bounded-distance core (rs63_*): syndromes r(alpha^i), i = 1..2t, of the zero-padded
// length-63 word, Massey's iteration, Chien search over all 63 positions (a "correction" that lands in the zero padding is
// accepted exactly like the reference does), Forney error values.  The decoders are bounded-distance, so any correct
// formulation returns the reference's symbols.  The Phase 2 decoder keeps the reference's own formulation: how it fails is
// pinned to it.  All per-lane polynomial arrays live in LDS as [index][lane] (dynamic indexing of a private array would go to
// scratch).

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ddn_device.h"
#include "ddn_gf64_dev.h"

using namespace ddn_gf64;

namespace {

// ---- the RS(63) bounded-distance core ---------------------------------------------------------------------------------------------
// This lane's LDS columns, element k at base[k * 64].  Every function starts from what its predecessor left, so a lane can decode
// one word after another in the same columns.
struct Rs63Work {
    uint8_t* W;   // [n_par + n_data] the word, parity symbols first
    uint8_t* S;   // [1 + 2t] syndromes S_1 .. S_2t at their own index
    uint8_t* C;   // [18] Massey's connection polynomial
    uint8_t* B;   // [18] ... at its last length change
    uint8_t* Om;  // [16] the evaluator
    uint8_t* Loc; // [deg locator] root positions } in columns that are dead once the locator is final, never the locator's own
    uint8_t* Val; // [deg locator] errata values  }
    __device__ __forceinline__ uint8_t& w(int k) const { return W[k * 64]; }
    __device__ __forceinline__ uint8_t& s(int k) const { return S[k * 64]; }
    __device__ __forceinline__ uint8_t& c(int k) const { return C[k * 64]; }
    __device__ __forceinline__ uint8_t& b(int k) const { return B[k * 64]; }
    __device__ __forceinline__ uint8_t& om(int k) const { return Om[k * 64]; }
    __device__ __forceinline__ uint8_t& loc(int k) const { return Loc[k * 64]; }
    __device__ __forceinline__ uint8_t& val(int k) const { return Val[k * 64]; }
};

__device__ __forceinline__ void
rs63_load(const Rs63Work& wk, const uint8_t* dp, const uint8_t* pp, int n_par, int n_data) {
    for (int k = 0; k < n_par + n_data; k++) {
        wk.w(k) = (uint8_t)hex_pack((k < n_par) ? (pp + 6 * k) : (dp + 6 * (k - n_par)));
    }
}

// the data symbols back to bits (normalises non-0/1 bytes)
__device__ __forceinline__ void
rs63_store(const Rs63Work& wk, uint8_t* dp, int n_par, int n_data) {
    for (int k = 0; k < n_data; k++) {
        hex_unpack(wk.w(n_par + k), dp + 6 * k);
    }
}

// S_i = r(alpha^i), i = 1..n2; returns non-zero when any is
__device__ __forceinline__ int
rs63_syndromes(const Gf& gf, const Rs63Work& wk, int nsym, int n2) {
    int any = 0;
    for (int s = 1; s <= n2; s++) {
        int acc = 0;
        for (int j = 0; j < nsym; j++) {
            acc ^= gf.mul_exp(wk.w(j), (s * j) % 63);
        }
        wk.s(s) = (uint8_t)acc;
        any |= acc;
    }
    return any;
}

// Massey on the syndrome window sy[0 .. ns) (a column like the others) -> C; returns (L << 8) | degree of C
__device__ __forceinline__ int
rs63_massey(const Gf& gf, const Rs63Work& wk, const uint8_t* sy, int ns) {
    for (int k = 0; k < 18; k++) {
        wk.c(k) = (k == 0);
        wk.b(k) = (k == 0);
    }
    int L = 0, m = 1, b = 1;
    for (int it = 0; it < ns; it++) {
        int d = sy[it * 64];
        for (int k = 1; k <= L; k++) {
            d ^= gf.mul(wk.c(k), sy[(it - k) * 64]);
        }
        if (d == 0) {
            m++;
            continue;
        }
        const int f = gf.div(d, b);
        const bool grow = 2 * L <= it;
        // C += f x^m B and, on a length change, B = the old C (held in registers: static indices)
        uint8_t c_old[18];
#pragma unroll
        for (int k = 0; k < 18; k++) {
            c_old[k] = wk.c(k);
        }
        for (int k = 0; k + m < 18; k++) {
            wk.c(k + m) ^= (uint8_t)gf.mul(f, wk.b(k));
        }
        if (grow) {
            L = it + 1 - L;
#pragma unroll
            for (int k = 0; k < 18; k++) {
                wk.b(k) = c_old[k];
            }
            b = d;
            m = 1;
        } else {
            m++;
        }
    }
    int deg = 0;
    for (int k = 17; k >= 0; k--) {
        if (wk.c(k)) {
            deg = k;
            break;
        }
    }
    return (L << 8) | deg;
}

// roots of lam (degree ldeg) over the whole length-63 word: error at position p <-> lam(alpha^-p) = 0 -> Loc; returns the count
__device__ __forceinline__ int
rs63_chien(const Gf& gf, const Rs63Work& wk, const uint8_t* lam, int ldeg) {
    int nl = 0;
    for (int p = 0; p < 63; p++) {
        const int xi = (63 - p) % 63;
        int v = 0;
        for (int k = 0; k <= ldeg; k++) {
            v ^= gf.mul_exp(lam[k * 64], (k * xi) % 63);
        }
        if (v == 0) {
            if (nl < ldeg) { // (a polynomial has no more roots than its degree)
                wk.loc(nl) = (uint8_t)p;
            }
            nl++;
        }
    }
    return nl;
}

// errata values at Loc[0 .. nl) by Forney -> Val; false if a derivative vanishes.  The word is not touched here: every value is
// known before rs63_apply() takes the first.
__device__ __forceinline__ bool
rs63_forney(const Gf& gf, const Rs63Work& wk, const uint8_t* lam, int ldeg, int nl, int n2) {
    for (int k = 0; k < n2; k++) {
        int v = 0;
        for (int j = 0; j <= k && j <= ldeg; j++) {
            v ^= gf.mul(lam[j * 64], wk.s(k - j + 1));
        }
        wk.om(k) = (uint8_t)v;
    }
    for (int e = 0; e < nl; e++) {
        const int xi = (63 - wk.loc(e)) % 63;
        int num = 0, den = 0;
        for (int k = 0; k < n2; k++) {
            num ^= gf.mul_exp(wk.om(k), (k * xi) % 63);
        }
        for (int k = 1; k <= ldeg; k += 2) {
            den ^= gf.mul_exp(lam[k * 64], ((k - 1) * xi) % 63);
        }
        if (den == 0) {
            return false;
        }
        wk.val(e) = (uint8_t)gf.div(num, den);
    }
    return true;
}

__device__ __forceinline__ void
rs63_apply(const Rs63Work& wk, int nl, int nsym) {
    for (int e = 0; e < nl; e++) {
        const int p = wk.loc(e);
        if (p < nsym) {
            wk.w(p) ^= wk.val(e);
        }
    }
}

// errors only, up to t of them: corrects the word and returns true, or leaves it as it is
__device__ __forceinline__ bool
rs63_hard(const Gf& gf, const Rs63Work& wk, int t, int nsym) {
    const int r = rs63_massey(gf, wk, wk.S + 64, 2 * t);
    const int L = r >> 8, deg = r & 255;
    if (L > t || deg != L || rs63_chien(gf, wk, wk.C, L) != L || !rs63_forney(gf, wk, wk.C, L, L, 2 * t)) {
        return false;
    }
    rs63_apply(wk, L, nsym);
    return true;
}

} // namespace

// hard decision.  Clean, corrected or failed, the data bits are rewritten from the symbols (a failed word's from the uncorrected
// ones).  The roots and values sit in the two halves of B: t <= 8.
__global__ __launch_bounds__(64) void
k_rs63(uint8_t* __restrict__ data6, const uint8_t* __restrict__ parity6, int n_par, int n_data, int t, int n,
       uint8_t* __restrict__ status, DdnSel sel) {
    __shared__ uint8_t ex[128], lg[64];
    __shared__ uint8_t W[36][64], S[17][64], Cc[18][64], Bb[18][64], Om[16][64];
    const int lane = threadIdx.x;
    gf_fill_wg(ex, lg);
    const Gf gf = {ex, lg};
    const Rs63Work wk = {&W[0][lane], &S[0][lane], &Cc[0][lane], &Bb[0][lane], &Om[0][lane], &Bb[0][lane], &Bb[8][lane]};
    auto one = [&](long i) {
    uint8_t* dp = data6 + (size_t)i * n_data * 6;
    rs63_load(wk, dp, parity6 + (size_t)i * n_par * 6, n_par, n_data);
    const int nsym = n_par + n_data;
    int rc = 0;
    if (rs63_syndromes(gf, wk, nsym, 2 * t)) {
        rc = rs63_hard(gf, wk, t, nsym) ? 0 : 1;
    }
    rs63_store(wk, dp, n_par, n_data);
    status[i] = (uint8_t)rc;
    };
    ddn_sel_for_each(sel, (long)n, one);
}

// ---- RS errors-and-erasures with reliability-ranked erasures ------------------------------------------------------------
// == p25p1_rs_24_12_13_soft_reliability / _24_16_9_ / _36_20_17_ (src/protocol/p25/phase1/p25p1_rs_soft_reliability.cpp,
// p25p1_check_ldu.cpp:70-94, p25p1_check_hdu.cpp:48-69; DSDReedSolomon_*::decode_soft and ReedSolomon_63::decode_with_erasures,
// include/dsd-neo/fec/ReedSolomon.hpp:175-262,585-690,774-802; ranking p25p1_soft.cpp:86-168).
// Per codeword: hard decode; if that fails, the symbols are ranked by (reliability, position) and the n = 1, 2, ... weakest
// are declared erasures until an errors-and-erasures decode succeeds (n up to max(#below-threshold, t), capped at 2t).
// One attempt = erasure locator (grown by one factor per attempt), modified syndromes, Massey on the last 2t - n of
// them, 2v + n <= 2t, combined locator, Chien over the 63 positions (root count = degree, every erasure a root), errata
// values by Forney (the reference solves the equivalent Vandermonde system), and all 2t syndromes of the corrected word
// must vanish - updated from the received word's syndromes instead of recomputed.  On failure the data is untouched.
// The roots go to B and the values to M: both are dead once Massey has run on M's window.
__global__ __launch_bounds__(64) void
k_rs63_soft(uint8_t* __restrict__ data6, const uint8_t* __restrict__ parity6, const uint8_t* __restrict__ data_rel,
            const uint8_t* __restrict__ parity_rel, int n_par, int n_data, int t, int threshold, int n,
            uint8_t* __restrict__ status) {
    __shared__ uint8_t ex[128], lg[64];
    __shared__ uint8_t W[36][64], S[17][64], G[18][64], M[17][64], Cc[18][64], Bb[18][64], Lam[18][64], Om[16][64], Er[16][64];
    __shared__ uint16_t Key[36][64];
    const int lane = threadIdx.x;
    gf_fill_wg(ex, lg);
    const int i = blockIdx.x * 64 + lane;
    if (i >= n) {
        return;
    }
    const Gf gf = {ex, lg};
    const Rs63Work wk = {&W[0][lane], &S[0][lane], &Cc[0][lane], &Bb[0][lane], &Om[0][lane], &Bb[0][lane], &M[0][lane]};
    const int nsym = n_par + n_data, n2 = 2 * t;
    uint8_t* dp = data6 + (size_t)i * n_data * 6;
    rs63_load(wk, dp, parity6 + (size_t)i * n_par * 6, n_par, n_data);
    int rc = 1;
    if (!rs63_syndromes(gf, wk, nsym, n2) || rs63_hard(gf, wk, t, nsym)) {
        rc = 0;
        rs63_store(wk, dp, n_par, n_data);
    }
    if (rc != 0) {
        // rank the symbols: (reliability, position) ascending; position = parity index, then n_par + data index
        int hits = 0;
        for (int k = 0; k < nsym; k++) {
            const int rel = (k < n_par) ? parity_rel[(size_t)i * n_par + k] : data_rel[(size_t)i * n_data + (k - n_par)];
            hits += rel < threshold;
            Key[k][lane] = (uint16_t)(rel * 64 + k);
        }
        int nr = hits > t ? hits : t;
        nr = nr > nsym ? nsym : nr;
        nr = nr > n2 ? n2 : nr;
        for (int j = 0; j < nr; j++) { // selection of the nr smallest keys, in order
            int bk = 0x7fffffff, bi = 0;
            for (int k = 0; k < nsym; k++) {
                const int kk = Key[k][lane];
                if (kk < bk) {
                    bk = kk;
                    bi = k;
                }
            }
            Key[bi][lane] = 0xFFFF;
            Er[j][lane] = (uint8_t)bi;
        }
        for (int k = 0; k < 18; k++) {
            G[k][lane] = (k == 0);
        }
        for (int ne = 1; ne <= nr && rc != 0; ne++) {
            // erasure locator grows by (1 + alpha^pos x)
            const int f = ex[Er[ne - 1][lane] % 63];
            for (int k = ne - 1; k >= 0; k--) {
                G[k + 1][lane] ^= (uint8_t)gf.mul(G[k][lane], f);
            }
            for (int k = 0; k < n2; k++) {
                int v = 0;
                for (int j = 0; j <= ne && j <= k; j++) {
                    v ^= gf.mul(G[j][lane], S[k - j + 1][lane]);
                }
                M[k][lane] = (uint8_t)v;
            }
            const int udeg = rs63_massey(gf, wk, &M[ne][lane], n2 - ne) & 255;
            if (2 * udeg + ne > n2) {
                continue;
            }
            int gdeg = 0;
            for (int k = 17; k >= 0; k--) {
                if (G[k][lane]) {
                    gdeg = k;
                    break;
                }
            }
            if (gdeg + udeg > n2) {
                continue;
            }
            for (int k = 0; k < 18; k++) {
                Lam[k][lane] = 0;
            }
            for (int a = 0; a <= gdeg; a++) {
                for (int b = 0; b <= udeg; b++) {
                    Lam[a + b][lane] ^= (uint8_t)gf.mul(G[a][lane], Cc[b][lane]);
                }
            }
            int ldeg = 0;
            for (int k = 17; k >= 0; k--) {
                if (Lam[k][lane]) {
                    ldeg = k;
                    break;
                }
            }
            const int nl = (ldeg > 0) ? rs63_chien(gf, wk, &Lam[0][lane], ldeg) : 0;
            if (nl != ldeg || nl > n2) {
                continue;
            }
            bool cover = true;
            for (int e = 0; e < ne; e++) {
                bool ok = false;
                for (int k = 0; k < nl; k++) {
                    ok |= (wk.loc(k) == Er[e][lane]);
                }
                cover &= ok;
            }
            if (!cover || !rs63_forney(gf, wk, &Lam[0][lane], ldeg, nl, n2)) {
                continue;
            }
            // every syndrome of the corrected word must vanish: S_s ^ sum_k val_k alpha^(s loc_k)
            int resid = 0;
            for (int s2 = 1; s2 <= n2; s2++) {
                int v = S[s2][lane];
                for (int k = 0; k < nl; k++) {
                    v ^= gf.mul_exp(wk.val(k), (s2 * wk.loc(k)) % 63);
                }
                resid |= v;
            }
            if (resid) {
                continue;
            }
            rc = 0;
            rs63_apply(wk, nl, nsym);
            rs63_store(wk, dp, n_par, n_data);
        }
    }
    status[i] = (uint8_t)rc;
}

extern "C" hipError_t
ddn_dev_rs63(uint8_t* data6, const uint8_t* parity6, int n_par, int n_data, int t, int n, uint8_t* status,
             hipStream_t st) {
    if (n <= 0) {
        return hipSuccess;
    }
    const DdnSel sel = ddn_sel_for(1);
    hipLaunchKernelGGL(k_rs63, dim3(ddn_sel_grid(&sel, ((unsigned long)n + 63) / 64)), dim3(64), 0, st, data6, parity6, n_par, n_data, t, n,
                       status, sel);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_rs63_soft(uint8_t* data6, const uint8_t* parity6, const uint8_t* data_rel, const uint8_t* parity_rel, int n_par,
                  int n_data, int t, int threshold, int n, uint8_t* status, hipStream_t st) {
    if (n <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_rs63_soft, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, data6, parity6, data_rel, parity_rel,
                       n_par, n_data, t, threshold, n, status);
    return hipGetLastError();
}

// ---- P25 Phase 2 RS(63,35) sections with caller-given erasures --------------------------------------------------------------
// == ez_rs28_ess / _facch / _sacch (src/fec/ez.cpp:104-281) over the vendored ezpwd RS<63,35> (GF(64) from x^6+x+1, roots
// alpha^1..alpha^28; decoder src/third_party/ezpwd/rs_base:1380-1720): block position p carries the coefficient of
// x^(62-p); syndromes, erasure locator, Berlekamp's iteration from step n_erasures + 1 with the length rule
// 2 L <= r + n_erasures - 1, Chien search over the 63 positions stopped at deg(lambda) roots, Forney from the last root to
// the first.  A root count short of the degree, a zero derivative or a non-zero value inside the pad fails the decode (-1)
// and leaves the section as received (the reference decodes a copy and copies back on a positive count only).
// One section per thread, its polynomials in LDS columns.
namespace {
constexpr int R28 = 28;

__host__ __device__ inline int
rs28_n_data(int kind) { // 0 ESS, 1 FACCH, 2 SACCH
    return kind == 0 ? 16 : (kind == 1 ? 26 : 30);
}

// a batch of sections as every kernel of the family sees it
struct Rs28Sections {
    int kind;
    uint8_t* payload_bits;     // [n][n_data * 6], corrected in place
    const uint8_t* parity_bits;
    const int8_t* erasures;    // [n][28] positions less the pad, the ranked lists' fixed erasures first
    const uint8_t* n_erasures; // [n] list lengths, or null: none
    int n;
    int32_t* status;           // [n] located symbols, or -1
    uint8_t* used_dynamic;     // [n] set where a retry decoded, or null
};

// one of them
struct Rs28Block {
    uint8_t* pl;
    const uint8_t* pa;
    const int8_t* er;
    int n_list, n_data, n_par, first, pad; // the data symbols sit at block positions first .. 34, the parity from 35
};

__device__ __forceinline__ Rs28Block
rs28_block(const Rs28Sections& s, int i) {
    Rs28Block b;
    b.n_data = rs28_n_data(s.kind);
    b.n_par = s.kind == 0 ? 28 : (s.kind == 1 ? 19 : 22);
    b.first = 35 - b.n_data;
    b.pad = s.kind == 0 ? 19 : 0;
    b.pl = s.payload_bits + (size_t)i * b.n_data * 6;
    b.pa = s.parity_bits + (size_t)i * b.n_par * 6;
    b.er = s.erasures + (size_t)i * R28;
    const int nl = s.n_erasures ? (int)s.n_erasures[i] : 0;
    b.n_list = nl > R28 ? R28 : nl;
    return b;
}

struct Rs28Work { // this lane's LDS columns, element k at base[k * 64]
    uint8_t* Cw;  // [63] the block
    uint8_t* Sy;  // [28]
    uint8_t* La;  // [29]
    uint8_t* Bp;  // [29]
    uint8_t* Tp;  // [29]
    uint8_t* Om;  // [28]
    uint8_t* Rt;  // [28]
    __device__ __forceinline__ uint8_t& cw(int k) const { return Cw[k * 64]; }
    __device__ __forceinline__ uint8_t& sy(int k) const { return Sy[k * 64]; }
    __device__ __forceinline__ uint8_t& la(int k) const { return La[k * 64]; }
    __device__ __forceinline__ uint8_t& bp(int k) const { return Bp[k * 64]; }
    __device__ __forceinline__ uint8_t& tp(int k) const { return Tp[k * 64]; }
    __device__ __forceinline__ uint8_t& om(int k) const { return Om[k * 64]; }
    __device__ __forceinline__ uint8_t& rt(int k) const { return Rt[k * 64]; }
};
__device__ __forceinline__ void
rs28_load(const Rs28Work& wk, const Rs28Block& blk) { // the block as received, one symbol per LDS row
    for (int p = 0; p < blk.first; p++) {
        wk.cw(p) = 0;
    }
    for (int k = 0; k < blk.n_data; k++) {
        wk.cw(blk.first + k) = (uint8_t)hex_pack(blk.pl + 6 * k);
    }
    for (int k = 0; k < blk.n_par; k++) {
        wk.cw(35 + k) = (uint8_t)hex_pack(blk.pa + 6 * k);
    }
    for (int p = 35 + blk.n_par; p < 63; p++) {
        wk.cw(p) = 0;
    }
}

__device__ __forceinline__ void
rs28_store(const Rs28Work& wk, const Rs28Block& blk) {
    for (int k = 0; k < blk.n_data; k++) {
        hex_unpack(wk.cw(blk.first + k), blk.pl + 6 * k);
    }
}

// by Horner; returns non-zero when any is
__device__ __forceinline__ int
rs28_syndromes(const Gf& gf, const Rs28Work& wk) {
    int any = 0;
#pragma unroll // (r + 1 a constant: the reduction mod 63 inside mul_exp becomes a compare and a subtract)
    for (int r = 0; r < R28; r++) {
        int v = 0;
        for (int p = 0; p < 63; p++) {
            v = gf.mul_exp(v, r + 1) ^ wk.cw(p);
        }
        wk.sy(r) = (uint8_t)v;
        any |= v;
    }
    return any;
}

// One attempt: the received block (syndromes in Sy, not all zero) with the first n_er erasures of its list -> located symbols and
// the corrected block in Cw, or -1 and Cw in no defined state.  Only Forney's step reads the block: cw_ready says Cw holds it as
// received, otherwise it is taken (again) when the decode gets that far.
__device__ __forceinline__ int
rs28_attempt(const Gf& gf, const Rs28Work& wk, const Rs28Block& blk, int n_er, bool cw_ready) {
    constexpr int R = R28;
    for (int k = 0; k <= R; k++) {
        wk.la(k) = k == 0 ? 1 : 0;
    }
    for (int e = 0; e < n_er; e++) {
        const int bp = (int)blk.er[e] + blk.pad; // block position
        const int X = gf.ex[(((62 - bp) % 63) + 63) % 63];
        for (int j = e + 1; j > 0; j--) {
            wk.la(j) ^= (uint8_t)gf.mul(wk.la(j - 1), X);
        }
    }
    for (int k = 0; k <= R; k++) {
        wk.bp(k) = wk.la(k);
    }
    int el = n_er;
    for (int r = n_er + 1; r <= R; r++) {
        int d = 0;
        for (int k = 0; k < r; k++) {
            d ^= gf.mul(wk.la(k), wk.sy(r - k - 1));
        }
        if (d == 0) {
            for (int k = R; k > 0; k--) {
                wk.bp(k) = wk.bp(k - 1);
            }
            wk.bp(0) = 0;
            continue;
        }
        wk.tp(0) = wk.la(0);
        for (int k = 0; k < R; k++) {
            wk.tp(k + 1) = wk.la(k + 1) ^ (uint8_t)gf.mul(d, wk.bp(k));
        }
        if (2 * el <= r + n_er - 1) {
            el = r + n_er - el;
            for (int k = 0; k <= R; k++) {
                wk.bp(k) = (uint8_t)gf.div(wk.la(k), d);
            }
        } else {
            for (int k = R; k > 0; k--) {
                wk.bp(k) = wk.bp(k - 1);
            }
            wk.bp(0) = 0;
        }
        for (int k = 0; k <= R; k++) {
            wk.la(k) = wk.tp(k);
        }
    }
    int deg = 0;
    for (int k = 0; k <= R; k++) {
        deg = wk.la(k) ? k : deg;
    }
    int count = 0;
    for (int r = 1; r <= 63 && count < deg; r++) {
        int q = 1;
        for (int j = 1; j <= deg; j++) {
            q ^= gf.mul_exp(wk.la(j), r * j);
        }
        if (q == 0) {
            wk.rt(count) = (uint8_t)r;
            count++;
        }
    }
    if (count != deg || deg == 0) {
        return -1;
    }
    for (int k = 0; k < deg; k++) {
        int v = 0;
        for (int j = 0; j <= k; j++) {
            v ^= gf.mul(wk.sy(k - j), wk.la(j));
        }
        wk.om(k) = (uint8_t)v;
    }
    const int top = (deg < R - 1 ? deg : R - 1) & ~1;
    if (!cw_ready) {
        rs28_load(wk, blk);
    }
    for (int j = count - 1; j >= 0; j--) {
        const int rt = wk.rt(j), loc = rt - 1;
        int num = 0, den = 0;
        for (int k = 0; k < deg; k++) {
            num ^= gf.mul_exp(wk.om(k), k * rt);
        }
        for (int k = top; k >= 0; k -= 2) {
            den ^= gf.mul_exp(wk.la(k + 1), k * rt);
        }
        if (den == 0 || (num != 0 && loc < blk.pad)) {
            return -1;
        }
        if (num != 0) {
            wk.cw(loc) ^= (uint8_t)gf.div(num, den);
        }
    }
    return count;
}
} // namespace

// The decode of every section with the first n_fixed erasures of its list (all of a list that is shorter), and in the same thread
// the ranked retries add_lo .. add_hi (p25p2_decode_facch_ranked()): attempt a takes n_fixed + a erasures, every one starts from the
// block as received, the first that decodes is taken, and the list's end stops them.  A pass that starts at a retry (add_lo > 0)
// visits the sections that have failed so far and whose list reaches that far.  ess_rule: a plain decode (attempt 0) that located
// 15 or more symbols is not taken (p25p2_ess_decode_with_soft_erasures(), p25p2_frame.c:1063-1066).
__global__ __launch_bounds__(64) void
k_rs28_decode(Rs28Sections s, int n_fixed, int add_lo, int add_hi, int ess_rule) {
    __shared__ uint8_t ex[128], lg[64];
    __shared__ uint8_t Cw[63][64], Sy[R28][64], La[R28 + 1][64], Bp[R28 + 1][64], Tp[R28 + 1][64], Om[R28][64], Rt[R28][64];
    const int lane = threadIdx.x;
    gf_fill_wg(ex, lg);
    const Gf gf = {ex, lg};
    const Rs28Work wk = {&Cw[0][lane], &Sy[0][lane], &La[0][lane], &Bp[0][lane], &Tp[0][lane], &Om[0][lane], &Rt[0][lane]};
    const int i = blockIdx.x * 64 + lane;
    if (i >= s.n) {
        return;
    }
    const Rs28Block blk = rs28_block(s, i);
    if (add_lo > 0 && (s.status[i] >= 0 || n_fixed + add_lo > blk.n_list)) {
        return;
    }
    rs28_load(wk, blk);
    if (!rs28_syndromes(gf, wk)) {
        s.status[i] = 0;
        return;
    }
    int result = -1;
    for (int att = add_lo;; att++) {
        const int n_er = n_fixed + att < blk.n_list ? n_fixed + att : blk.n_list;
        result = rs28_attempt(gf, wk, blk, n_er, att == add_lo);
        if (ess_rule && att == 0 && result >= 15) {
            result = -1;
        }
        if (result >= 0) {
            rs28_store(wk, blk);
            if (att > 0 && s.used_dynamic) {
                s.used_dynamic[i] = 1;
            }
            break;
        }
        if (att >= add_hi || n_fixed + att + 1 > blk.n_list) {
            break;
        }
    }
    s.status[i] = result;
}

// The retries of a section are independent of each other (attempt a decodes the received block with the first n_fixed + a erasures of
// the ranked list; the reference takes the first that succeeds), so they can run side by side instead of one after the other - one
// decode deep instead of up to max_add.  The syndromes do not depend on the attempt: this pass leaves those of every failed section
// in syn [n][28].
__global__ __launch_bounds__(64) void
k_rs28_syn(Rs28Sections s, uint8_t* __restrict__ syn) {
    __shared__ uint8_t ex[128], lg[64];
    __shared__ uint8_t Cw[63][64], Sy[R28][64];
    const int lane = threadIdx.x;
    gf_fill_wg(ex, lg);
    const Gf gf = {ex, lg};
    const Rs28Work wk = {&Cw[0][lane], &Sy[0][lane], nullptr, nullptr, nullptr, nullptr, nullptr};
    const int i = blockIdx.x * 64 + lane;
    if (i >= s.n || s.status[i] >= 0) {
        return;
    }
    rs28_load(wk, rs28_block(s, i));
    rs28_syndromes(gf, wk);
    for (int r = 0; r < R28; r++) {
        syn[(size_t)i * R28 + r] = wk.sy(r);
    }
}

// ... and this one gives every (failed section, attempt 1 .. max_add) pair a thread that decodes on its own, from the syndromes on
// file (it reads the code word only when its decode reaches Forney's step), and leaves its verdict in probe_res [pair] (-2: the list
// ends before this attempt) and, when it succeeded, the corrected data symbols in stage [pair][n_data]
__global__ __launch_bounds__(64) void
k_rs28_probe(Rs28Sections s, int n_fixed, int max_add, const uint8_t* __restrict__ syn, int32_t* __restrict__ probe_res,
             uint8_t* __restrict__ stage) {
    __shared__ uint8_t ex[128], lg[64];
    __shared__ uint8_t Cw[63][64], Sy[R28][64], La[R28 + 1][64], Bp[R28 + 1][64], Tp[R28 + 1][64], Om[R28][64], Rt[R28][64];
    const int lane = threadIdx.x;
    gf_fill_wg(ex, lg);
    const Gf gf = {ex, lg};
    const Rs28Work wk = {&Cw[0][lane], &Sy[0][lane], &La[0][lane], &Bp[0][lane], &Tp[0][lane], &Om[0][lane], &Rt[0][lane]};
    const long gid = (long)blockIdx.x * 64 + lane;
    const int i = (int)(gid / max_add), add = 1 + (int)(gid % max_add);
    if (i >= s.n || s.status[i] >= 0) {
        return;
    }
    const Rs28Block blk = rs28_block(s, i);
    if (n_fixed + add > blk.n_list) {
        probe_res[gid] = -2;
        return;
    }
    for (int r = 0; r < R28; r++) {
        wk.sy(r) = syn[(size_t)i * R28 + r];
    }
    const int result = rs28_attempt(gf, wk, blk, n_fixed + add, false);
    if (result >= 0) {
        for (int k = 0; k < blk.n_data; k++) {
            stage[(size_t)gid * blk.n_data + k] = wk.cw(blk.first + k);
        }
    }
    probe_res[gid] = result;
}

// per failed section: the first attempt whose probe succeeded - its corrected data symbols become the payload, its count the status
__global__ __launch_bounds__(256) void
k_rs28_pick(int kind, uint8_t* __restrict__ payload_bits, int n, int32_t* __restrict__ status, uint8_t* __restrict__ used_dynamic, int probe_A,
            const int32_t* __restrict__ probe_res, const uint8_t* __restrict__ stage) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || status[i] >= 0) {
        return;
    }
    const int n_data = rs28_n_data(kind);
    for (int k = 0; k < probe_A; k++) {
        const int r = probe_res[(long)i * probe_A + k];
        if (r == -2) {
            return; // the list ends here: every due retry failed, the payload stays as received
        }
        if (r >= 0) {
            const uint8_t* sy = stage + ((size_t)i * probe_A + k) * n_data;
            uint8_t* pl = payload_bits + (size_t)i * n_data * 6;
            for (int d = 0; d < n_data; d++) {
                hex_unpack(sy[d], pl + 6 * d);
            }
            status[i] = r;
            if (used_dynamic) {
                used_dynamic[i] = 1;
            }
            return;
        }
    }
}

static void
rs28_decode(const Rs28Sections& s, int n_fixed, int add_lo, int add_hi, int ess_rule, hipStream_t st) {
    hipLaunchKernelGGL(k_rs28_decode, dim3((unsigned)((s.n + 63) / 64)), dim3(64), 0, st, s, n_fixed, add_lo, add_hi, ess_rule);
}

// the retries 1 .. max_add of every failed section: side by side (syndromes on file, probe pass over (section, attempt) pairs, pick)
// or one after the other in the section's thread
static hipError_t
rs28_retries(const Rs28Sections& s, int n_fixed, int max_add, hipStream_t st) {
    // Side by side costs more decodes in total (every due attempt of a failed section runs, not only those up to the first success)
    // and buys depth - a decode is ~0.5 ms deep for its thread however many run: measured on one MI355X, 4096 channels x 6 groups of
    // Phase 2 traffic (12 k - 30 k sections per call) and 65 536 ESS sections (lists up to 28 deep) gain, 65 536 FACCH bursts (655 k
    // pairs, lists 10 deep: the device is already full) lose - so very large batches of short lists keep the loop in the thread.
    const int n = s.n;
    const long pairs = (long)n * max_add;
    if (pairs > 600000 && max_add < 28) {
        rs28_decode(s, n_fixed, 1, max_add, 0, st);
        return hipGetLastError();
    }
    const int n_data = rs28_n_data(s.kind);
    int32_t* res = nullptr;
    hipError_t e = hipMallocAsync((void**)&res, (size_t)pairs * sizeof(int32_t) + (size_t)n * 28 + (size_t)pairs * n_data, st);
    if (e != hipSuccess) {
        return e;
    }
    uint8_t* syn = (uint8_t*)(res + pairs);
    uint8_t* stage = syn + (size_t)n * 28;
    hipLaunchKernelGGL(k_rs28_syn, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, s, syn);
    hipLaunchKernelGGL(k_rs28_probe, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, st, s, n_fixed, max_add, (const uint8_t*)syn, res,
                       stage);
    hipLaunchKernelGGL(k_rs28_pick, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s.kind, s.payload_bits, n, s.status, s.used_dynamic,
                       max_add, (const int32_t*)res, (const uint8_t*)stage);
    e = hipGetLastError();
    const hipError_t f = hipFreeAsync(res, st);
    return e != hipSuccess ? e : f;
}

// caller-given erasures: every listed one is fixed, no retries
extern "C" hipError_t
ddn_dev_rs28(int kind, uint8_t* payload_bits, const uint8_t* parity_bits, const int8_t* erasures, const uint8_t* n_erasures,
             int n, int32_t* status, hipStream_t st) {
    if (n <= 0) {
        return hipSuccess;
    }
    rs28_decode(Rs28Sections{kind, payload_bits, parity_bits, erasures, n_erasures, n, status, nullptr}, R28, 0, 0, 0, st);
    return hipGetLastError();
}

// the Phase 2 stages' decode (ddn_p25p2_burst.hip): with the fixed erasures for every section, then the failed sections' retries
extern "C" hipError_t
ddn_rs28_ranked(int kind, uint8_t* payload_bits, const uint8_t* parity_bits, const int8_t* erasures28, const uint8_t* n_total, int n,
                int32_t* status, uint8_t* used_dynamic, int n_fixed, int max_add, int ess_rule, hipStream_t st) {
    const Rs28Sections s = {kind, payload_bits, parity_bits, erasures28, n_total, n, status, used_dynamic};
    rs28_decode(s, n_fixed, 0, 0, ess_rule, st);
    return rs28_retries(s, n_fixed, max_add, st);
}
