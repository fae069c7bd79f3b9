/* oracle/ddn_oracle_mbe.c - TEST INFRASTRUCTURE ONLY (see oracle/README.md): CPU restatement of the vocoder stage.
 *
 * PARITY UNPINNED for everything past the frame FEC decode.  dsd-neo calls the un-vendored dependency mbelib-neo 2.0.0
 * @ 6138cce7091d90e4be9e889ac166006265d3e8fb (vcpkg-ports/mbe-neo/portfile.cmake:5-7; call sites
 * src/core/vocoder/dsd_mbe.c:152-190,540-598); its source is not under /root/reference.  This file restates the
 * PUBLISHED algorithm of the mbelib lineage (mbelib 1.3, ISC licence: ecc.c, imbe7200x4400.c, ambe3600x2450.c,
 * mbelib.c) behind the entry points the reference is witnessed to use (CMakeLists.txt:626-657):
 *
 *   om_imbe7200x4400_decode / om_ambe3600x2450_decode   frame FEC - PINNED: the four capture-derived IMBE vectors of
 *       tests/core/test_core_mbe_transform_context.c:134-152 decode to the words and correction counts that test
 *       asserts (:886 "FC00000000000000000000 err=[2]", :869 excluded_corrections 10, :1014 0, :1020 8, :1043 12),
 *       see tests/test_oracle_mbe.py.  The AMBE frame decode has no absolute vector in the reference (its tests compare
 *       the library with itself); only the b0 bit positions are witnessed (same file :228-238).
 *   om_process   parameter unpack -> enhancement -> synthesis: structure per mbelib 1.3; quantiser tables come in as a
 *       ddn_mbe_tables blob (include/ddn_mbe.h); libm / rand() replaced as ddn_oracle_mbe_math.h explains.
 */
#include <string.h>

#include "../include/ddn_mbe.h"
#include "ddn_oracle_mbe_math.h"

/* ---- Golay(23,12), generator x^11+x^10+x^6+x^5+x^4+x^2+1 (mbelib ecc_const: golayGenerator 0x63a..0x475 are
 * x^(11+i) mod g), and Hamming(15,11) with mbelib's parity masks ---- */
#define GOLAY_G 0xC75u

static uint32_t
golay_syndrome(uint32_t w23) {
    for (int i = 22; i >= 11; i--) {
        if ((w23 >> i) & 1u) {
            w23 ^= GOLAY_G << (i - 11);
        }
    }
    return w23 & 0x7FFu;
}

static uint32_t g_golay_tab[2048];
static int g_golay_ready;

static void
golay_build(void) {
    if (g_golay_ready) {
        return;
    }
    g_golay_tab[0] = 0;
    for (int a = 0; a < 23; a++) {
        for (int b = a; b < 23; b++) {
            for (int c = b; c < 23; c++) {
                const uint32_t e = (1u << a) | (1u << b) | (1u << c);
                g_golay_tab[golay_syndrome(e)] = e;
            }
        }
    }
    g_golay_ready = 1;
}

/* mbe_golay2312 (mbelib ecc.c): in[22] is the codeword's MSB, data bits in[22..11]; the parity bits are left as
 * received; returns the number of DATA bits changed */
static int
golay2312(uint8_t* v /* [23], in place */) {
    uint32_t block = 0;
    for (int i = 22; i >= 0; i--) {
        block = (block << 1) | (v[i] & 1u);
    }
    const uint32_t e = g_golay_tab[golay_syndrome(block)];
    int errs = 0;
    for (int i = 22; i >= 11; i--) {
        if ((e >> i) & 1u) {
            v[i] ^= 1u;
            errs++;
        }
    }
    return errs;
}

static const uint16_t k_hamming_mask[4] = {0x7f08, 0x78e4, 0x66d2, 0x55b1};

/* mbe_hamming1511: v[14] MSB; single-error correction over all 15 bits, returns 0 / 1 */
static int
hamming1511(uint8_t* v /* [15] */) {
    uint32_t block = 0;
    for (int i = 14; i >= 0; i--) {
        block = (block << 1) | (v[i] & 1u);
    }
    uint32_t syn = 0;
    for (int i = 0; i < 4; i++) {
        syn = (syn << 1) | (uint32_t)(__builtin_popcount(block & k_hamming_mask[i]) & 1);
    }
    if (!syn) {
        return 0;
    }
    for (int p = 0; p < 15; p++) {
        uint32_t col = 0;
        for (int i = 0; i < 4; i++) {
            col = (col << 1) | ((k_hamming_mask[i] >> p) & 1u);
        }
        if (col == syn) {
            v[p] ^= 1u;
            break;
        }
    }
    return 1;
}

/* pseudo-random modulation sequence (mbe_demodulateImbe7200x4400Data): pr[0] = 16 * u0, pr[i] = 173 pr[i-1] + 13849
 * mod 65536, bit = pr >> 15 */
static void
pn_bits(uint32_t seed12, int n, uint8_t* out /* [n + 1], out[0] unused */) {
    uint32_t pr = (16u * seed12) & 0xFFFFu;
    for (int i = 1; i <= n; i++) {
        pr = (173u * pr + 13849u) & 0xFFFFu;
        out[i] = (uint8_t)(pr >> 15);
    }
}

static void
set_result(int32_t res[5], unsigned flags, int c0, int c4, int total) {
    res[0] = (int32_t)flags;
    res[1] = c0;
    res[2] = c4;
    res[3] = total;
    res[4] = total - c0;
}

/* mbe_decodeImbe7200x4400Frame = mbe_eccImbe7200x4400C0 + mbe_demodulateImbe7200x4400Data + mbe_eccImbe7200x4400Data */
int
om_imbe7200x4400_decode(const uint8_t* fr /* [8][23] */, int soft, uint8_t* imbe_d /* [88] */, int32_t* res /* [5] */) {
    golay_build();
    uint8_t f[8][23];
    for (int i = 0; i < 8 * 23; i++) {
        if (fr[i] > 1) {
            return MBE_STATUS_INVALID_BITS;
        }
        f[i / 23][i % 23] = fr[i];
    }
    const int c0 = golay2312(f[0]);
    uint32_t u0 = 0;
    for (int i = 22; i >= 11; i--) {
        u0 = (u0 << 1) | f[0][i];
    }
    uint8_t pr[115];
    pn_bits(u0, 114, pr);
    int k = 1;
    for (int i = 1; i < 4; i++) {
        for (int j = 22; j >= 0; j--) {
            f[i][j] ^= pr[k++];
        }
    }
    for (int i = 4; i < 7; i++) {
        for (int j = 14; j >= 0; j--) {
            f[i][j] ^= pr[k++];
        }
    }
    int total = c0, c4 = 0, o = 0;
    for (int j = 22; j > 10; j--) {
        imbe_d[o++] = f[0][j];
    }
    for (int i = 1; i < 4; i++) {
        total += golay2312(f[i]);
        for (int j = 22; j > 10; j--) {
            imbe_d[o++] = f[i][j];
        }
    }
    for (int i = 4; i < 7; i++) {
        const int e = hamming1511(f[i]);
        if (i == 4) {
            c4 = e;
        }
        total += e;
        for (int j = 14; j >= 4; j--) {
            imbe_d[o++] = f[i][j];
        }
    }
    for (int j = 6; j >= 0; j--) {
        imbe_d[o++] = f[7][j];
    }
    set_result(res, MBE_PROCESS_FLAG_C0_VALID | MBE_PROCESS_FLAG_C4_VALID | (soft ? MBE_PROCESS_FLAG_SOFT_INPUT : 0u), c0,
               c4, total);
    return MBE_STATUS_OK;
}

/* mbe_decodeAmbe3600x2450Frame = mbe_eccAmbe3600x2450C0 + mbe_demodulateAmbe3600x2450Data + mbe_eccAmbe3600x2450Data:
 * c0 = ambe_fr[0][1..23] Golay(23,12) (bit 0 is the overall parity of the (24,12) word, not used), c1 = ambe_fr[1][0..22]
 * de-scrambled then Golay(23,12), c2 (11 bits) and c3 (14 bits) unprotected */
int
om_ambe3600x2450_decode(const uint8_t* fr /* [4][24] */, int soft, uint8_t* ambe_d /* [49] */, int32_t* res) {
    golay_build();
    uint8_t f[4][24];
    for (int i = 0; i < 96; i++) {
        if (fr[i] > 1) {
            return MBE_STATUS_INVALID_BITS;
        }
        f[i / 24][i % 24] = fr[i];
    }
    const int c0 = golay2312(&f[0][1]);
    uint32_t u0 = 0;
    for (int i = 23; i >= 12; i--) {
        u0 = (u0 << 1) | f[0][i];
    }
    uint8_t pr[24];
    pn_bits(u0, 23, pr);
    int k = 1;
    for (int j = 22; j >= 0; j--) {
        f[1][j] ^= pr[k++];
    }
    int o = 0;
    for (int j = 23; j > 11; j--) {
        ambe_d[o++] = f[0][j];
    }
    const int c1 = golay2312(f[1]);
    for (int j = 22; j > 10; j--) {
        ambe_d[o++] = f[1][j];
    }
    for (int j = 10; j >= 0; j--) {
        ambe_d[o++] = f[2][j];
    }
    for (int j = 13; j >= 0; j--) {
        ambe_d[o++] = f[3][j];
    }
    set_result(res, MBE_PROCESS_FLAG_C0_VALID | (soft ? MBE_PROCESS_FLAG_SOFT_INPUT : 0u), c0, 0, c0 + c1);
    return MBE_STATUS_OK;
}

/* ---- decoder history (mbelib.c: mbe_initMbeParms / mbe_moveMbeParms / mbe_useLastMbeParms) ---- */
void
om_init_parms(mbe_parms* cur, mbe_parms* prev, mbe_parms* enh) {
    memset(prev, 0, sizeof(*prev));
    prev->w0 = 0.09378f;
    prev->L = 30;
    prev->K = 10;
    prev->gamma = 0.0f;
    for (int l = 0; l <= 56; l++) {
        prev->Ml[l] = 0.0f;
        prev->Vl[l] = 0;
        prev->log2Ml[l] = 0.0f;
        prev->PHIl[l] = 0.0f;
        prev->PSIl[l] = OM_PI_F / 2.0f;
    }
    prev->repeat = 0;
    prev->un = 0;
    *cur = *prev;
    *enh = *prev;
}

static uint32_t
field_value(const uint8_t* d, const uint8_t (*order)[2], int n_bits, int field) {
    uint32_t v = 0;
    for (int p = 0; p < n_bits; p++) {
        if (order[p][0] == field && d[p]) {
            v |= 1u << order[p][1];
        }
    }
    return v;
}

static float
dequant(uint32_t b, int bits, float step) {
    if (bits <= 0) {
        return 0.0f;
    }
    return step * (((float)b - (float)(1u << (bits - 1))) + 0.5f);
}

/* log-magnitude prediction shared by both codecs (imbe7200x4400.c / ambe3600x2450.c, "eq. 75-79 / 185-190") */
static void
predict(const float* Tl, int L, const mbe_parms* prev, float rho, float extra, float* log2Ml) {
    float pl[59];
    const int pL = prev->L;
    for (int l = 0; l <= 58; l++) {
        pl[l] = (l <= 56) ? prev->log2Ml[l] : 0.0f;
    }
    pl[0] = pl[1];
    for (int l = pL + 1; l <= 58; l++) {
        pl[l] = pl[pL];
    }
    float sum = 0.0f;
    const float ratio = (float)pL / (float)L;
    for (int l = 1; l <= L; l++) {
        const float kl = ratio * (float)l;
        const int ki = (int)kl;
        const float dl = kl - (float)ki;
        sum = sum + (((1.0f - dl) * pl[ki]) + (dl * pl[ki + 1]));
    }
    sum = sum * (rho / (float)L);
    for (int l = 1; l <= L; l++) {
        const float kl = ratio * (float)l;
        const int ki = (int)kl;
        const float dl = kl - (float)ki;
        log2Ml[l] = (((Tl[l] + ((rho * (1.0f - dl)) * pl[ki])) + ((rho * dl) * pl[ki + 1])) - sum) + extra;
    }
}

/* inverse DCT of one block: c(j) = sum_k a(k) C(k) cos(pi (k-1)(j-1/2) / J), a(1) = 1 else 2 */
static float
idct_term(const float* C /* 1-based */, int J, int j) {
    float acc = 0.0f;
    for (int k = 1; k <= J; k++) {
        const float a = (k == 1) ? 1.0f : 2.0f;
        const float ang = (OM_PI_F * (float)(k - 1) * ((float)j - 0.5f)) / (float)J;
        acc = acc + (a * C[k]) * om_cosf(ang);
    }
    return acc;
}

/* mbe_decodeImbe4400Parms: 0 = ok, 1 = invalid fundamental */
static int
imbe_decode_parms(const uint8_t* d, const ddn_mbe_tables* T, mbe_parms* cur, const mbe_parms* prev) {
    cur->repeat = prev->repeat;
    uint32_t b0 = 0;
    for (int i = 0; i < 6; i++) {
        b0 = (b0 << 1) | d[i];
    }
    b0 = (b0 << 2) | ((uint32_t)d[85] << 1) | d[86];
    if (b0 > 207) {
        return 1;
    }
    cur->w0 = (4.0f * OM_PI_F) / ((float)b0 + 39.5f);
    /* L = (int)(0.9254 * (int)(pi / w0 + 0.25)) with pi / w0 = (b0 + 39.5) / 4, in exact integer arithmetic */
    const int t = (2 * (int)b0 + 81) / 8;
    const int L = (9254 * t) / 10000;
    if (L > 56 || L < 9) {
        return 1;
    }
    cur->L = L;
    const int K = (L < 37) ? (L + 2) / 3 : 12;
    cur->K = K;
    const uint8_t(*order)[2] = T->imbe_bit_order[L - 9];
    const uint8_t* bits = T->imbe_bits[L - 9];
    const uint32_t b1 = field_value(d, order, 88, 1);
    for (int l = 1; l <= L; l++) {
        int band = (l + 2) / 3;
        if (band > K) {
            band = K;
        }
        cur->Vl[l] = (int)((b1 >> (K - band)) & 1u);
    }
    float Gm[7];
    Gm[1] = T->imbe_gain_b2[field_value(d, order, 88, 2) & 63u];
    for (int m = 2; m <= 6; m++) {
        const int B = bits[m + 1];
        Gm[m] = dequant(field_value(d, order, 88, m + 1), B, T->imbe_gain_step[B] * T->imbe_gain_sigma[m - 2]);
    }
    float Tl[57];
    int l = 1, field = 8;
    for (int i = 1; i <= 6; i++) {
        const int J = (L + i - 1) / 6;
        float C[12];
        C[1] = idct_term(Gm, 6, i);
        for (int k = 2; k <= J; k++, field++) {
            const int B = bits[field];
            const int ks = (k > 10) ? 10 : k;
            C[k] = dequant(field_value(d, order, 88, field), B, T->imbe_hoc_step[B] * T->imbe_hoc_sigma[ks - 2]);
        }
        for (int j = 1; j <= J; j++) {
            Tl[l++] = idct_term(C, J, j);
        }
    }
    float rho;
    if (L <= 15) {
        rho = 0.4f;
    } else if (L <= 24) {
        rho = (0.03f * (float)L) - 0.05f;
    } else {
        rho = 0.7f;
    }
    predict(Tl, L, prev, rho, 0.0f, cur->log2Ml);
    for (l = 1; l <= L; l++) {
        cur->Ml[l] = om_expf(0.693f * cur->log2Ml[l]);
    }
    return 0;
}

/* mbe_decodeAmbe2450Parms: 0 = ok, 2 = erasure, 3 = tone; silence frames decode as ok */
static int
ambe_decode_parms(const uint8_t* d, const ddn_mbe_tables* T, mbe_parms* cur, const mbe_parms* prev, unsigned* flags) {
    cur->repeat = prev->repeat;
    const uint32_t b0 = ((uint32_t)d[0] << 6) | ((uint32_t)d[1] << 5) | ((uint32_t)d[2] << 4) | ((uint32_t)d[3] << 3)
                        | ((uint32_t)d[37] << 2) | ((uint32_t)d[38] << 1) | d[39];
    if (b0 >= 120 && b0 <= 123) {
        *flags |= MBE_PROCESS_FLAG_ERASURE;
        return 2;
    }
    if (b0 == 126 || b0 == 127) {
        *flags |= MBE_PROCESS_FLAG_TONE;
        return 3;
    }
    int silence = 0;
    float f0;
    int L;
    if (b0 == 124 || b0 == 125) {
        silence = 1;
        *flags |= MBE_PROCESS_FLAG_SILENCE;
        cur->w0 = OM_TWO_PI_F / 32.0f;
        f0 = 1.0f / 32.0f;
        L = 14;
    } else {
        f0 = T->ambe_f0[b0];
        cur->w0 = f0 * OM_TWO_PI_F;
        L = T->ambe_L[b0];
    }
    cur->L = L;
    const float unvc = 0.2046f / sqrtf(cur->w0);
    const uint32_t b1 = ((uint32_t)d[4] << 4) | ((uint32_t)d[5] << 3) | ((uint32_t)d[6] << 2) | ((uint32_t)d[7] << 1) | d[35];
    const uint32_t b2 = ((uint32_t)d[8] << 4) | ((uint32_t)d[9] << 3) | ((uint32_t)d[10] << 2) | ((uint32_t)d[11] << 1) | d[36];
    uint32_t b3 = 0, b4 = 0, b5 = 0, b6 = 0, b7 = 0, b8 = 0;
    for (int i = 12; i <= 19; i++) {
        b3 = (b3 << 1) | d[i];
    }
    b3 = (b3 << 1) | d[40];
    for (int i = 20; i <= 23; i++) {
        b4 = (b4 << 1) | d[i];
    }
    b4 = (b4 << 3) | ((uint32_t)d[41] << 2) | ((uint32_t)d[42] << 1) | d[43];
    for (int i = 24; i <= 27; i++) {
        b5 = (b5 << 1) | d[i];
    }
    b5 = (b5 << 1) | d[44];
    b6 = ((uint32_t)d[28] << 3) | ((uint32_t)d[29] << 2) | ((uint32_t)d[30] << 1) | d[45];
    b7 = ((uint32_t)d[31] << 3) | ((uint32_t)d[32] << 2) | ((uint32_t)d[33] << 1) | d[46];
    b8 = ((uint32_t)d[34] << 2) | ((uint32_t)d[47] << 1) | d[48];
    for (int l = 1; l <= L; l++) {
        if (silence) {
            cur->Vl[l] = 0;
        } else {
            int jl = (int)((float)l * 16.0f * f0);
            if (jl > 7) {
                jl = 7;
            }
            cur->Vl[l] = T->ambe_vuv[b1][jl];
        }
    }
    cur->gamma = T->ambe_dg[b2] + (0.5f * prev->gamma);
    float Gm[9];
    Gm[1] = 0.0f;
    for (int i = 0; i < 3; i++) {
        Gm[2 + i] = T->ambe_prba24[b3][i];
    }
    for (int i = 0; i < 4; i++) {
        Gm[5 + i] = T->ambe_prba58[b4][i];
    }
    float Ri[9];
    for (int i = 1; i <= 8; i++) {
        Ri[i] = idct_term(Gm, 8, i);
    }
    const float rconst = 0.353553390593274f; /* 1 / (2 sqrt 2) */
    float Cik[5][7];
    memset(Cik, 0, sizeof(Cik));
    for (int i = 1; i <= 4; i++) {
        Cik[i][1] = 0.5f * (Ri[2 * i - 1] + Ri[2 * i]);
        Cik[i][2] = rconst * (Ri[2 * i - 1] - Ri[2 * i]);
    }
    const float* hoc[5] = {0, T->ambe_hoc5[b5], T->ambe_hoc6[b6], T->ambe_hoc7[b7], T->ambe_hoc8[b8]};
    float Tl[57];
    int l = 1;
    float tsum = 0.0f;
    for (int i = 1; i <= 4; i++) {
        const int J = T->ambe_blocks[L][i - 1];
        for (int k = 3; k <= J && k <= 6; k++) {
            Cik[i][k] = hoc[i][k - 3];
        }
        float C[58];
        for (int k = 1; k <= J; k++) {
            C[k] = (k <= 6) ? Cik[i][k] : 0.0f;
        }
        for (int j = 1; j <= J; j++) {
            Tl[l] = idct_term(C, J, j);
            tsum = tsum + Tl[l];
            l++;
        }
    }
    /* BigGamma = gamma - 0.5 log2(L) - mean(Tl)  (ambe3600x2450.c "eq. 185") */
    const float big_gamma = (cur->gamma - (0.5f * (logf((float)L) / logf(2.0f)))) - (tsum / (float)L);
    predict(Tl, L, prev, 0.65f, big_gamma, cur->log2Ml);
    for (l = 1; l <= L; l++) {
        const float m = om_expf(0.693f * cur->log2Ml[l]);
        cur->Ml[l] = cur->Vl[l] ? m : unvc * m;
    }
    return 0;
}

/* mbe_spectralAmpEnhance (mbelib.c) */
static void
enhance(mbe_parms* cur) {
    const int L = cur->L;
    float Rm0 = 0.0f, Rm1 = 0.0f;
    for (int l = 1; l <= L; l++) {
        const float m2 = cur->Ml[l] * cur->Ml[l];
        Rm0 = Rm0 + m2;
        Rm1 = Rm1 + (m2 * om_cosf(cur->w0 * (float)l));
    }
    const float R2m0 = Rm0 * Rm0, R2m1 = Rm1 * Rm1;
    float sum = 0.0f;
    for (int l = 1; l <= L; l++) {
        float W = 1.0f;
        if (cur->Ml[l] != 0.0f) {
            const float num = (0.96f * OM_PI_F) * ((R2m0 + R2m1) - (((2.0f * Rm0) * Rm1) * om_cosf(cur->w0 * (float)l)));
            const float den = (cur->w0 * Rm0) * (R2m0 - R2m1);
            const float x = num / den;
            if ((8 * l) <= L || !(x > 0.0f) || !(x < 3.0e38f)) {
                W = 1.0f;
            } else {
                const float tmp = sqrtf(cur->Ml[l]) * sqrtf(sqrtf(x));
                W = (tmp > 1.2f) ? 1.2f : ((tmp < 0.5f) ? 0.5f : tmp);
            }
            cur->Ml[l] = cur->Ml[l] * W;
        }
        sum = sum + (cur->Ml[l] * cur->Ml[l]);
    }
    const float gamma = (sum == 0.0f) ? 1.0f : sqrtf(Rm0 / sum);
    for (int l = 1; l <= L; l++) {
        cur->Ml[l] = gamma * cur->Ml[l];
    }
}

static float
unvoiced_mix(float w0, float w0l, int l, int n, uint32_t base, uint32_t tag) {
    float c3 = 0.0f;
    for (int i = 0; i < 3; i++) {
        const float rph = om_rand_phase(om_mix(base, tag + (uint32_t)i));
        c3 = c3 + om_cosf(((w0 * (float)n) * (((float)l + ((float)i * OM_UVSTEP)) - OM_UVOFFSET)) + rph);
        if (w0l > OM_UVTHRESHOLD) {
            c3 = c3 + (((w0l - OM_UVTHRESHOLD) * OM_UVRAND) * om_u01(om_mix(om_mix(base, tag + 0x40u + (uint32_t)i), (uint32_t)n)));
        }
    }
    return c3;
}

/* mbe_synthesizeSpeechf (mbelib.c), uvquality 3; seed / frame number key the random phases and noise */
static void
synthesize(float* out, mbe_parms* cur, mbe_parms* prev, uint32_t seed, uint32_t frame_no) {
    const int N = 160;
    int num_uv = 0;
    for (int l = 1; l <= cur->L; l++) {
        if (cur->Vl[l] == 0) {
            num_uv++;
        }
    }
    const float cw0 = cur->w0, pw0 = prev->w0;
    int maxl;
    if (cur->L > prev->L) {
        maxl = cur->L;
        for (int l = prev->L + 1; l <= maxl; l++) {
            prev->Ml[l] = 0.0f;
            prev->Vl[l] = 1;
        }
    } else {
        maxl = prev->L;
        for (int l = cur->L + 1; l <= maxl; l++) {
            cur->Ml[l] = 0.0f;
            cur->Vl[l] = 1;
        }
    }
    const uint32_t fbase = om_mix(om_mix(0x9E3779B9u, seed), frame_no);
    for (int l = 1; l <= 56; l++) {
        /* phase track, wrapped to (-pi, pi] so that the cosine arguments stay small (mbelib lets it grow) */
        float psi = prev->PSIl[l] + ((pw0 + cw0) * ((float)(l * N) / 2.0f));
        psi = fmaf(-rintf(psi * 0.159154943091895336f), OM_TWO_PI_F, psi);
        cur->PSIl[l] = psi;
        if (l <= (cur->L / 4)) {
            cur->PHIl[l] = psi;
        } else {
            cur->PHIl[l] = psi + (((float)num_uv * om_rand_phase(om_mix(om_mix(fbase, (uint32_t)l), 0x100u))) / (float)cur->L);
        }
    }
    for (int n = 0; n < N; n++) {
        float acc = 0.0f;
        const float wp = om_ws(n + N), wc = om_ws(n);
        for (int l = 1; l <= maxl; l++) {
            const float cw0l = cw0 * (float)l, pw0l = pw0 * (float)l;
            const uint32_t base = om_mix(fbase, (uint32_t)l);
            const int cv = cur->Vl[l], pv = prev->Vl[l];
            if (cv == 0 && pv == 1) {
                const float c1 = (wp * prev->Ml[l]) * om_cosf((pw0l * (float)n) + prev->PHIl[l]);
                float c3 = unvoiced_mix(cw0, cw0l, l, n, base, 0x200u);
                c3 = (((c3 * OM_UVSINE) * wc) * cur->Ml[l]) * OM_QFACTOR;
                acc = acc + (c1 + c3);
            } else if (cv == 1 && pv == 0) {
                const float c1 = (wc * cur->Ml[l]) * om_cosf((cw0l * (float)(n - N)) + cur->PHIl[l]);
                float c3 = unvoiced_mix(pw0, pw0l, l, n, base, 0x300u);
                c3 = (((c3 * OM_UVSINE) * wp) * prev->Ml[l]) * OM_QFACTOR;
                acc = acc + (c1 + c3);
            } else if (cv == 1 || pv == 1) {
                const float c1 = (wp * prev->Ml[l]) * om_cosf((pw0l * (float)n) + prev->PHIl[l]);
                const float c2 = (wc * cur->Ml[l]) * om_cosf((cw0l * (float)(n - N)) + cur->PHIl[l]);
                acc = acc + (c1 + c2);
            } else {
                float c3 = unvoiced_mix(pw0, pw0l, l, n, base, 0x300u);
                c3 = (((c3 * OM_UVSINE) * wp) * prev->Ml[l]) * OM_QFACTOR;
                float c4 = unvoiced_mix(cw0, cw0l, l, n, base, 0x200u);
                c4 = (((c4 * OM_UVSINE) * wc) * cur->Ml[l]) * OM_QFACTOR;
                acc = acc + (c3 + c4);
            }
        }
        out[n] = acc;
    }
}

/* dsd_mbe.c:447-463 mbe_p25p1_is_tail_erasure (clear-mode teardown frame): FC prefix, <= 24 set bits, >= 10 corrections */
static int
p25p1_tail_erasure(const uint8_t* d, int corrections) {
    if (corrections < 10) {
        return 0;
    }
    unsigned prefix = 0;
    int set = 0;
    for (int i = 0; i < 88; i++) {
        if (i < 8) {
            prefix = (prefix << 1) | (d[i] & 1u);
        }
        set += d[i] & 1;
    }
    return prefix == 0xFCu && set <= 24;
}

/* mbe_processImbe4400Dataf / mbe_processAmbe2450Dataf (imbe7200x4400.c / ambe3600x2450.c) on one frame.
 * res_in may be NULL (no errors).  cur->un carries the talk path's frame number. */
int
om_process(int codec, const ddn_mbe_tables* T, const uint8_t* bits, const int32_t* res_in, int tail_rule, uint32_t seed,
           float* pcm, int32_t* res_out, mbe_parms* cur, mbe_parms* prev, mbe_parms* enh) {
    int32_t r[5] = {0, 0, 0, 0, 0};
    if (res_in) {
        memcpy(r, res_in, sizeof(r));
    }
    unsigned flags = (unsigned)r[0];
    const int errs2 = r[3];
    const int n_bits = codec == DDN_MBE_IMBE_7200X4400 ? 88 : 49;
    for (int i = 0; i < n_bits; i++) {
        if (bits[i] > 1) {
            memset(pcm, 0, sizeof(float) * 160);
            return MBE_STATUS_INVALID_BITS;
        }
    }
    if (tail_rule && codec == DDN_MBE_IMBE_7200X4400 && p25p1_tail_erasure(bits, errs2)) {
        memset(pcm, 0, sizeof(float) * 160);
        if (res_out) {
            set_result(res_out, 0u, 0, 0, 0); /* clear_mbe_status, dsd_mbe.c:562 */
        }
        return MBE_STATUS_OK;
    }
    const uint32_t frame_no = (uint32_t)cur->un;
    int bad;
    if (codec == DDN_MBE_IMBE_7200X4400) {
        bad = imbe_decode_parms(bits, T, cur, prev);
        if (bad == 1 || errs2 > 5) {
            const int un = cur->un;
            *cur = *prev; /* mbe_useLastMbeParms */
            cur->un = un;
            cur->repeat++;
            flags |= MBE_PROCESS_FLAG_REPEAT;
        } else {
            cur->repeat = 0;
        }
    } else {
        bad = ambe_decode_parms(bits, T, cur, prev, &flags);
        if (bad == 2 || bad == 3) {
            cur->repeat = 0;
        } else if (errs2 > 3) {
            const int un = cur->un;
            *cur = *prev;
            cur->un = un;
            cur->repeat++;
            flags |= MBE_PROCESS_FLAG_REPEAT;
        } else {
            cur->repeat = 0;
        }
    }
    /* mbelib 1.3 imbe7200x4400.c mbe_processImbe4400Dataf: `if (cur_mp->repeat <= 3)` alone; ambe3600x2450.c
     * mbe_processAmbe2450Dataf: `if ((bad == 0) && (cur_mp->repeat <= 3))` */
    if ((codec == DDN_MBE_IMBE_7200X4400 || bad == 0) && cur->repeat <= 3) {
        const int un = cur->un;
        *prev = *cur; /* mbe_moveMbeParms (cur, prev) */
        enhance(cur);
        synthesize(pcm, cur, enh, seed, frame_no);
        *enh = *cur;
        cur->un = prev->un = enh->un = (int)((uint32_t)un + 1u); /* the counter wraps as the device's uint32 does */
    } else {
        const int un = cur->un;
        flags |= MBE_PROCESS_FLAG_MUTE;
        memset(pcm, 0, sizeof(float) * 160);
        om_init_parms(cur, prev, enh);
        cur->un = prev->un = enh->un = (int)((uint32_t)un + 1u); /* the counter wraps as the device's uint32 does */
    }
    if (res_out) {
        res_out[0] = (int32_t)flags;
        res_out[1] = r[1];
        res_out[2] = r[2];
        res_out[3] = r[3];
        res_out[4] = r[4];
    }
    return MBE_STATUS_OK;
}

/* [S][F] frames, talk path s seeded with seed0 + s; state arrays cur / prev / enh are [S] */
int
om_process_batch(int codec, const ddn_mbe_tables* T, const uint8_t* bits, const int32_t* res_in, int tail_rule,
                 uint32_t seed0, int S, int F, float* pcm, int32_t* res_out, mbe_parms* cur, mbe_parms* prev,
                 mbe_parms* enh) {
    const int nb = codec == DDN_MBE_IMBE_7200X4400 ? 88 : 49;
    for (int s = 0; s < S; s++) {
        for (int f = 0; f < F; f++) {
            const size_t i = (size_t)s * (size_t)F + (size_t)f;
            const int rc = om_process(codec, T, bits + i * (size_t)nb, res_in ? res_in + i * 5 : 0, tail_rule, seed0 + (uint32_t)s,
                                      pcm + i * 160, res_out ? res_out + i * 5 : 0, cur + s, prev + s, enh + s);
            if (rc != MBE_STATUS_OK) {
                return rc;
            }
        }
    }
    return MBE_STATUS_OK;
}
