// ddn_m17_dev.h - device helpers shared by the M17 frame decoders (ddn_m17.hip: link setup and stream frames; ddn_m17_data.hip: packet
// and BERT frames): the randomiser sequence, soft_symbol_to_viterbi_cost() and the search for a channel's j-th sync of a kind.
// Include it inside the translation unit's anonymous namespace.
#ifndef DDN_M17_DEV_H
#define DDN_M17_DEV_H

// M17 specification, "Randomizer": 46 bytes, most significant bit first (== m17_scramble[], src/protocol/m17/m17_tables.c:16-27)
__constant__ uint8_t k_m17_rand[46] = {0xD6, 0xB5, 0xE2, 0x30, 0x82, 0xFF, 0x84, 0x62, 0xBA, 0x4E, 0x96, 0x90, 0xD8, 0x98, 0xDD, 0x5D,
                                       0x0C, 0xC8, 0x52, 0x43, 0x91, 0x1D, 0xF8, 0x6E, 0x68, 0x2F, 0x35, 0xDA, 0x14, 0xEA, 0xCD, 0x76,
                                       0x19, 0x8D, 0xD5, 0x80, 0xD1, 0x33, 0x87, 0x13, 0x57, 0x18, 0x2D, 0x29, 0x78, 0xC3};

__device__ __forceinline__ float
min_sq2(float x, float a, float b) {
    const float da = x - a, db = x - b;
    const float d2a = da * da, d2b = db * db;
    return d2a < d2b ? d2a : d2b;
}

// soft_symbol_to_viterbi_cost(): thr = {center, umid, lmid, max, min}; bit 0 = the dibit's high bit
__device__ __forceinline__ uint32_t
m17_soft_cost(float symbol, const float* thr, int bit) {
    float center = thr[0], umid = thr[1], lmid = thr[2], max_val = thr[3], min_val = thr[4];
    if (!(min_val < lmid && lmid < center && center < umid && umid < max_val)) {
        float span = max_val - min_val;
        if (span < 1e-3f) {
            span = 2.0f;
        }
        const float half = span * 0.5f;
        min_val = center - half;
        max_val = center + half;
        lmid = center - (span / 6.0f);
        umid = center + (span / 6.0f);
    }
    const float n3 = 0.5f * (min_val + lmid), n1 = 0.5f * (lmid + center), p1 = 0.5f * (center + umid), p3 = 0.5f * (umid + max_val);
    float sigma = (max_val - min_val) / 6.0f;
    if (sigma < 1e-3f) {
        sigma = 1e-3f;
    }
    const float inv_2sigma2 = 0.5f / (sigma * sigma);
    float d0, d1;
    if ((bit & 1) == 0) {
        d0 = min_sq2(symbol, p1, p3);
        d1 = min_sq2(symbol, n1, n3);
    } else {
        d0 = min_sq2(symbol, n1, p1);
        d1 = min_sq2(symbol, n3, p3);
    }
    const float llr = (d1 - d0) * inv_2sigma2;
    if (llr >= 16.0f) {
        return 0u;
    }
    if (llr <= -16.0f) {
        return 65535u;
    }
    const float pr1 = 1.0f / (1.0f + ddn_expf(llr));
    long long q = __float2ll_rn(pr1 * 65535.0f); // lrintf
    q = q < 0 ? 0 : (q > 65535 ? 65535 : q);
    return (uint32_t)q;
}

// the channel's j-th sync of one of two patterns whose 184 payload symbols lie inside the call's records (whole wavefront; -1: none)
__device__ __forceinline__ int
m17_find_sync(const int32_t* sync_pos, const uint8_t* sync_pat, int ns, int cnt, int j, int pat_a, int pat_b, int lane) {
    int found = -1, seen = 0;
    for (int k0 = 0; k0 < ns && found < 0; k0 += 64) {
        const int k = k0 + lane;
        bool is = false;
        if (k < ns) {
            const int pat = sync_pat[k];
            is = (pat == pat_a || pat == pat_b) && sync_pos[k] + 185 <= cnt;
        }
        const unsigned long long b = __ballot(is);
        const int nb = __popcll(b);
        if (seen + nb > j) {
            unsigned long long m = b;
            for (int q = 0; q < j - seen; q++) {
                m &= m - 1;
            }
            found = k0 + __ffsll((long long)m) - 1;
        }
        seen += nb;
    }
    return found;
}

#endif
