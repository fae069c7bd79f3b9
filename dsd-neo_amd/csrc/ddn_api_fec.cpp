// ddn_api_fec.cpp — C-ABI for the batched trellis / Viterbi decoders (include/ddn_hip.h, "FEC" section) and the
// single-codeword drop-in symbols with the reference's names.
//
// Batched calls take DEVICE pointers and a stream; `_host` variants check their arguments with their batched twin's check_*(),
// stage host buffers through the device (DdnStaged, synchronous) and run the twin.  Nothing here computes on the CPU: without a
// GPU every call with good arguments fails with DDN_ENODEV.

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "ddn_api_util.h"
#include "ddn_device.h"

namespace {
int
build_puncture(const uint8_t* punct, int p_len, int in_len, DdnPuncture* pu, int* u_len) {
    memset(pu, 0, sizeof(*pu));
    if (!punct || p_len <= 0) {
        *u_len = in_len;
        return DDN_OK;
    }
    if (p_len > 64) {
        ddn_set_error("puncture pattern longer than 64 entries");
        return DDN_ERANGE;
    }
    pu->p_len = p_len;
    int ones = 0;
    for (int r = 0; r < p_len; r++) {
        pu->keep[r] = punct[r] ? 1 : 0;
        pu->ones_before[r] = (uint8_t)ones;
        ones += pu->keep[r];
    }
    pu->ones_total = ones;
    if (ones == 0) {
        ddn_set_error("puncture pattern keeps nothing");
        return DDN_EINVAL;
    }
    int i = 0, u = 0, p = 0;
    while (i < in_len) { // same walk as viterbi_decode_punctured (reference src/core/util/dsd_misc.c:160-173)
        if (pu->keep[p]) {
            i++;
        }
        u++;
        p = (p + 1) % p_len;
    }
    *u_len = u;
    return DDN_OK;
}
} // namespace

static int
check_p25_12_soft(const char* who, const int16_t* llr196, const uint8_t* out12) {
    return (llr196 && out12) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_p25_12_soft_batch(const int16_t* d_llr196, size_t n, uint8_t* d_out12, int32_t* d_metric, void* hip_stream) {
    DDN_TRY(check_p25_12_soft(__func__, d_llr196, d_out12));
    HIP_TRY(ddn_dev_p25_half_rate(d_llr196, (int)n, d_out12, d_metric, (hipStream_t)hip_stream));
    return DDN_OK;
}

static int
check_r34(const char* who, const uint8_t* dibits98, const uint8_t* out18) {
    return (dibits98 && out18) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_r34_batch(const uint8_t* d_dibits98, const uint8_t* d_reliab98, size_t n, uint8_t* d_out18, void* hip_stream) {
    DDN_TRY(check_r34(__func__, d_dibits98, d_out18));
    HIP_TRY(ddn_dev_r34(d_dibits98, d_reliab98, (int)n, d_out18, (hipStream_t)hip_stream));
    return DDN_OK;
}

// (the length is also held against the LDS a workgroup may have on this device, before anything is staged or launched: sixteen code
// words of n_steps steps need 64 n_steps + 48 bytes in the hard form and 96 n_steps + 80 with reliabilities)
static int
check_nxdn_conv(const char* who, const uint8_t* sym, const uint8_t* rel, const uint8_t* out, int n_steps, int n_bits, int out_stride) {
    if (!(sym && out && n_steps > 0 && n_steps <= 1024 && n_bits >= 0 && n_bits <= n_steps && out_stride >= (n_bits + 7) / 8)) {
        return ddn_bad_argument(who);
    }
    size_t need = 0, limit = 0;
    HIP_TRY(ddn_dev_k5_nxdn_lds(n_steps, rel != nullptr, &need, &limit));
    if (need > limit) {
        ddn_set_error("%s: %d steps need %zu bytes of LDS per workgroup, the device offers %zu", who, n_steps, need, limit);
        return DDN_ERANGE;
    }
    return DDN_OK;
}

extern "C" int
ddn_fec_nxdn_conv_batch(const uint8_t* d_sym, const uint8_t* d_rel, size_t n, int n_steps, int n_bits,
                        uint16_t* d_metrics_io, uint8_t* d_out, int out_stride, void* hip_stream) {
    DDN_TRY(check_nxdn_conv(__func__, d_sym, d_rel, d_out, n_steps, n_bits, out_stride));
    HIP_TRY(ddn_dev_k5_nxdn(d_sym, d_rel, (int)n, n_steps, n_bits, d_metrics_io, d_out, out_stride,
                            (hipStream_t)hip_stream));
    return DDN_OK;
}

static int
check_viterbi_k5(const char* who, const uint16_t* soft, const uint8_t* out, int in_len, int out_stride) {
    return (soft && out && in_len >= 2 && out_stride > 0) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_viterbi_k5_batch(const uint16_t* d_soft, size_t n, int in_len, const uint8_t* punct, int p_len, uint8_t* d_out,
                         int out_stride, uint32_t* d_cost, void* hip_stream) {
    DDN_TRY(check_viterbi_k5("ddn_fec_viterbi_k5_batch", d_soft, d_out, in_len, out_stride));
    DdnPuncture pu;
    int u_len = 0;
    int rc = build_puncture(punct, p_len, in_len, &pu, &u_len);
    if (rc != DDN_OK) {
        return rc;
    }
    if (u_len > 244 * 2) {
        ddn_set_error("viterbi_k5: %d soft bits exceed the decoder's 244-step history", u_len);
        return DDN_ERANGE;
    }
    if (out_stride < (u_len / 2 + 3) / 8 + 1) {
        ddn_set_error("viterbi_k5: out_stride %d too small for %d steps", out_stride, u_len / 2);
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_k5_m17(d_soft, (int)n, in_len, u_len, &pu, d_out, out_stride, d_cost, (hipStream_t)hip_stream));
    return DDN_OK;
}

// the same for callers inside the library that know which code words they want (d_wanted [n], 0 = leave undecoded: the YSF payload's
// dense decode lists are mostly empty for one of the two block lengths)
extern "C" int
ddn_fec_viterbi_k5_batch_wanted(const uint16_t* d_soft, size_t n, int in_len, const uint8_t* punct, int p_len, uint8_t* d_out,
                                int out_stride, uint32_t* d_cost, const uint8_t* d_wanted, void* hip_stream) {
    DDN_TRY(check_viterbi_k5("ddn_fec_viterbi_k5_batch", d_soft, d_out, in_len, out_stride));
    DdnPuncture pu;
    int u_len = 0;
    int rc = build_puncture(punct, p_len, in_len, &pu, &u_len);
    if (rc != DDN_OK) {
        return rc;
    }
    if (u_len > 244 * 2 || out_stride < (u_len / 2 + 3) / 8 + 1) {
        ddn_set_error("viterbi_k5: %d soft bits / out_stride %d out of range", u_len, out_stride);
        return DDN_ERANGE;
    }
    HIP_TRY(ddn_dev_k5_m17_wanted(d_soft, (int)n, in_len, u_len, &pu, d_out, out_stride, d_cost, d_wanted, (hipStream_t)hip_stream));
    return DDN_OK;
}

static int
check_nid_decode(const char* who, const uint8_t* bits63, const int32_t* out4) {
    return (bits63 && out4) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_p25p1_nid_decode_batch(const uint8_t* d_bits63, const uint8_t* d_rel63, const int32_t* d_observed_nac,
                           const uint8_t* d_parity, const uint8_t* d_parity_rel, int erasure_threshold, size_t n,
                           int32_t* d_out4, void* hip_stream) {
    DDN_TRY(check_nid_decode(__func__, d_bits63, d_out4));
    HIP_TRY(ddn_dev_nid_decode(d_bits63, d_rel63, d_observed_nac, d_parity, d_parity_rel, erasure_threshold, (int)n,
                               d_out4, (hipStream_t)hip_stream));
    return DDN_OK;
}

static int
check_hamming_10_6_3(const char* who, const uint8_t* bits10, const uint8_t* errs) {
    return (bits10 && errs) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_hamming_10_6_3_batch(uint8_t* d_bits10, size_t n, uint8_t* d_errs, void* hip_stream) {
    DDN_TRY(check_hamming_10_6_3(__func__, d_bits10, d_errs));
    HIP_TRY(ddn_dev_hamming_10_6_3(d_bits10, (int)n, d_errs, (hipStream_t)hip_stream));
    return DDN_OK;
}

// ---- host-buffer variants ------------------------------------------------------------------------------
extern "C" int
ddn_fec_p25_12_soft_host(const int16_t* llr196, size_t n, uint8_t* out12, int32_t* metric) {
    DDN_TRY(check_p25_12_soft(__func__, llr196, out12));
    DdnStaged s;
    const int16_t* a = s.in(llr196, n * 196 * 2);
    uint8_t* b = s.out(out12, n * 12);
    int32_t* m = s.out(metric, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_p25_12_soft_batch(a, n, b, m, nullptr));
    return s.finish();
}

extern "C" int
ddn_fec_r34_host(const uint8_t* dibits98, const uint8_t* reliab98, size_t n, uint8_t* out18) {
    DDN_TRY(check_r34(__func__, dibits98, out18));
    DdnStaged s;
    const uint8_t* a = s.in(dibits98, n * 98);
    const uint8_t* r = s.in_opt(reliab98, n * 98);
    uint8_t* b = s.out(out18, n * 18);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_r34_batch(a, r, n, b, nullptr));
    return s.finish();
}

extern "C" int
ddn_fec_nxdn_conv_host(const uint8_t* sym, const uint8_t* rel, size_t n, int n_steps, int n_bits, uint16_t* metrics_io,
                       uint8_t* out, int out_stride) {
    DDN_TRY(check_nxdn_conv(__func__, sym, rel, out, n_steps, n_bits, out_stride));
    DdnStaged s;
    const uint8_t* a = s.in(sym, n * 2 * (size_t)n_steps);
    const uint8_t* r = s.in_opt(rel, n * 2 * (size_t)n_steps);
    uint16_t* m = metrics_io ? s.inout(metrics_io, n * 32) : nullptr;
    uint8_t* b = s.out(out, n * (size_t)out_stride);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_nxdn_conv_batch(a, r, n, n_steps, n_bits, m, b, out_stride, nullptr));
    return s.finish();
}

extern "C" int
ddn_fec_viterbi_k5_host(const uint16_t* soft, size_t n, int in_len, const uint8_t* punct, int p_len, uint8_t* out,
                        int out_stride, uint32_t* cost) {
    DDN_TRY(check_viterbi_k5(__func__, soft, out, in_len, out_stride));
    DdnStaged s;
    const uint16_t* a = s.in(soft, n * (size_t)in_len * 2);
    uint8_t* b = s.out(out, n * (size_t)out_stride);
    uint32_t* c = s.out(cost, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_viterbi_k5_batch(a, n, in_len, punct, p_len, b, out_stride, c, nullptr));
    return s.finish();
}

extern "C" int
ddn_p25p1_nid_decode_host(const uint8_t* bits63, const uint8_t* rel63, const int32_t* observed_nac,
                          const uint8_t* parity, const uint8_t* parity_rel, int erasure_threshold, size_t n,
                          int32_t* out4) {
    DDN_TRY(check_nid_decode(__func__, bits63, out4));
    DdnStaged s;
    const uint8_t* a = s.in(bits63, n * 63);
    const uint8_t* r = s.in_opt(rel63, n * 63);
    const int32_t* o = s.in_opt(observed_nac, n * 4);
    const uint8_t* p = s.in_opt(parity, n);
    const uint8_t* q = s.in_opt(parity_rel, n);
    int32_t* out = s.out(out4, n * 16);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25p1_nid_decode_batch(a, r, o, p, q, erasure_threshold, n, out, nullptr));
    return s.finish();
}

extern "C" int
ddn_fec_hamming_10_6_3_host(uint8_t* bits10, size_t n, uint8_t* errs) {
    DDN_TRY(check_hamming_10_6_3(__func__, bits10, errs));
    DdnStaged s;
    uint8_t* a = s.inout(bits10, n * 10);
    uint8_t* e = s.out(errs, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_hamming_10_6_3_batch(a, n, e, nullptr));
    return s.finish();
}

// reference: int hamming_10_6_3_decode(char* data, const char* parity)  (include/dsd-neo/fec/block_codes.h)
extern "C" int
hamming_10_6_3_decode(char* data, const char* parity) {
    if (!data || !parity) {
        return 2;
    }
    uint8_t b[10], e = 2;
    for (int i = 0; i < 6; i++) {
        b[i] = (uint8_t)data[i];
    }
    for (int i = 0; i < 4; i++) {
        b[6 + i] = (uint8_t)parity[i];
    }
    if (ddn_fec_hamming_10_6_3_host(b, 1, &e) != DDN_OK) {
        return 2;
    }
    if (e == 1) {
        for (int i = 0; i < 6; i++) {
            data[i] = (char)b[i];
        }
    }
    return e;
}

// C-ABI-safe shape of p25p1_nid_decode() (the reference returns a struct by value,
// include/dsd-neo/protocol/p25/p25p1_check_nid.h:38-39): out4 = {status, nac, duid, error_count}
extern "C" int
ddn_p25p1_nid_decode(const char bch_code[63], const uint8_t* reliab63, int observed_nac, unsigned char parity,
                     uint8_t parity_reliab, int erasure_threshold, int out4[4]) {
    if (!bch_code || !out4) {
        return DDN_EINVAL;
    }
    int32_t obs = observed_nac, o[4];
    int rc = ddn_p25p1_nid_decode_host((const uint8_t*)bch_code, reliab63, &obs, &parity, &parity_reliab,
                                       erasure_threshold, 1, o);
    for (int i = 0; i < 4 && rc == DDN_OK; i++) {
        out4[i] = o[i];
    }
    return rc;
}

// ---- drop-in single-codeword symbols (reference names) ---------------------------------------------------
// include/dsd-neo/protocol/p25/p25_12.h:21, include/dsd-neo/protocol/dmr/r34_viterbi.h:19-26,
// include/dsd-neo/fec/viterbi.h:23-25, include/dsd-neo/protocol/nxdn/nxdn_convolution.h:24-28
extern "C" int
p25_12_soft_llr(const uint8_t* input, const int16_t* bit_llr196, uint8_t treturn[12]) {
    (void)input;
    int32_t metric = 0;
    if (ddn_fec_p25_12_soft_host(bit_llr196, 1, treturn, &metric) != DDN_OK) {
        return -1;
    }
    return metric;
}

extern "C" int
dmr_r34_viterbi_decode(const uint8_t* dibits98, uint8_t out_bytes18[18]) {
    if (!dibits98 || !out_bytes18) {
        return -1;
    }
    return ddn_fec_r34_host(dibits98, nullptr, 1, out_bytes18) == DDN_OK ? 0 : -1;
}

extern "C" int
dmr_r34_viterbi_decode_soft(const uint8_t* dibits98, const uint8_t* reliab98, uint8_t out_bytes18[18]) {
    if (!dibits98 || !reliab98 || !out_bytes18) {
        return -1;
    }
    return ddn_fec_r34_host(dibits98, reliab98, 1, out_bytes18) == DDN_OK ? 0 : -1;
}

extern "C" uint32_t
viterbi_decode(uint8_t* out, const uint16_t* in, const uint16_t len) {
    uint32_t cost = 0;
    const int stride = (len / 2 + 3) / 8 + 1;
    std::vector<uint8_t> tmp((size_t)stride);
    if (ddn_fec_viterbi_k5_host(in, 1, len, nullptr, 0, tmp.data(), stride, &cost) != DDN_OK) {
        return 0xFFFFFFFFu;
    }
    memcpy(out, tmp.data(), (size_t)stride);
    return cost;
}

extern "C" uint32_t
viterbi_decode_punctured(uint8_t* out, const uint16_t* in, const uint8_t* punct, const uint16_t in_len,
                         const uint16_t p_len) {
    uint32_t cost = 0;
    DdnPuncture pu;
    int u_len = 0;
    if (build_puncture(punct, p_len, in_len, &pu, &u_len) != DDN_OK) {
        return 0xFFFFFFFFu;
    }
    const int stride = (u_len / 2 + 3) / 8 + 1;
    std::vector<uint8_t> tmp((size_t)stride);
    if (ddn_fec_viterbi_k5_host(in, 1, in_len, punct, p_len, tmp.data(), stride, &cost) != DDN_OK) {
        return 0xFFFFFFFFu;
    }
    memcpy(out, tmp.data(), (size_t)stride);
    return cost;
}

// Step-wise form of the same decoder (src/core/util/dsd_misc.c:188-283: viterbi_decode_bit updates file-static path
// metrics / history per symbol pair, viterbi_chainback walks them back, viterbi_reset clears them).  The drop-in keeps
// the symbol pairs per thread and runs the accumulated steps on the device at chainback time - the add-compare-select
// of step `pos` depends only on the pairs 0..pos, so the result is the one the incremental form reaches.
namespace {
thread_local std::vector<uint16_t> g_vb_soft;
} // namespace

extern "C" void
viterbi_reset(void) {
    g_vb_soft.clear();
}

extern "C" void
viterbi_decode_bit(uint16_t s0, uint16_t s1, const size_t pos) {
    if (pos >= 244) { // the reference's history array holds 244 steps
        return;
    }
    if (g_vb_soft.size() < 2 * (pos + 1)) {
        g_vb_soft.resize(2 * (pos + 1), 0x7FFF);
    }
    g_vb_soft[2 * pos] = s0;
    g_vb_soft[2 * pos + 1] = s1;
}

extern "C" uint32_t
viterbi_chainback(uint8_t* out, size_t pos, uint16_t len) {
    if (!out || pos == 0 || 2 * pos > g_vb_soft.size() || pos > 244) {
        return 0xFFFFFFFFu;
    }
    // viterbi_decode(out, in, 2 * pos) calls viterbi_chainback(out, pos, pos): bit position = step index + 4 there; a
    // caller's `len` only shifts where the bits land
    uint32_t cost = 0;
    const int stride = (int)((pos + 3) / 8 + 1);
    std::vector<uint8_t> tmp((size_t)stride);
    if (ddn_fec_viterbi_k5_host(g_vb_soft.data(), 1, (int)(2 * pos), nullptr, 0, tmp.data(), stride, &cost) != DDN_OK) {
        return 0xFFFFFFFFu;
    }
    if (len == pos) {
        memcpy(out, tmp.data(), (size_t)((len - 1) / 8 + 1) < (size_t)stride ? (size_t)stride : (size_t)((len - 1) / 8 + 1));
    } else {
        memset(out, 0, (size_t)((len - 1) / 8 + 1));
        for (size_t k = 0; k < pos; k++) { // step k's bit sits at k + 4 in tmp and at len + 4 - pos + k in `out`
            const size_t src = k + 4, dst = (size_t)len + 4 - pos + k;
            if ((tmp[src / 8] >> (7 - (src % 8))) & 1u) {
                out[dst / 8] |= (uint8_t)(1u << (7 - (dst % 8)));
            }
        }
    }
    return cost;
}

// The reference keeps the NXDN decoder's symbols-in-flight and path metrics in file-static storage
// (src/protocol/nxdn/nxdn_convolution.c:48-53); the drop-in keeps the same per-thread streaming contract and runs
// the accumulated steps on the device at chainback time.
namespace {
thread_local std::vector<uint8_t> g_nx_sym, g_nx_rel;
thread_local bool g_nx_soft = false;
thread_local uint16_t g_nx_metrics[16] = {0};
} // namespace

extern "C" void
CNXDNConvolution_init(void) {
    memset(g_nx_metrics, 0, sizeof(g_nx_metrics));
    g_nx_sym.clear();
    g_nx_rel.clear();
    g_nx_soft = false;
}

extern "C" void
CNXDNConvolution_start(void) {
    g_nx_sym.clear();
    g_nx_rel.clear();
    g_nx_soft = false;
}

extern "C" void
CNXDNConvolution_decode(uint8_t s0, uint8_t s1) {
    g_nx_sym.push_back(s0);
    g_nx_sym.push_back(s1);
    g_nx_rel.push_back(0);
    g_nx_rel.push_back(0);
}

extern "C" void
CNXDNConvolution_decode_soft(uint8_t s0, uint8_t s1, uint8_t r0, uint8_t r1) {
    g_nx_sym.push_back(s0);
    g_nx_sym.push_back(s1);
    g_nx_rel.push_back(r0);
    g_nx_rel.push_back(r1);
    g_nx_soft = true;
}

extern "C" void
CNXDNConvolution_chainback(unsigned char* out, unsigned int nBits) {
    const int n_steps = (int)(g_nx_sym.size() / 2);
    if (!out || n_steps <= 0 || (int)nBits > n_steps) {
        return;
    }
    const int stride = ((int)nBits + 7) / 8;
    std::vector<uint8_t> tmp((size_t)(stride > 0 ? stride : 1));
    if (ddn_fec_nxdn_conv_host(g_nx_sym.data(), g_nx_soft ? g_nx_rel.data() : nullptr, 1, n_steps, (int)nBits,
                               g_nx_metrics, tmp.data(), stride > 0 ? stride : 1)
        != DDN_OK) {
        return;
    }
    // the reference writes exactly nBits bits and leaves the rest of the last byte alone
    for (unsigned int i = 0; i < nBits; i++) {
        const uint8_t mask = (uint8_t)(0x80u >> (i & 7));
        if (tmp[i >> 3] & mask) {
            out[i >> 3] |= mask;
        } else {
            out[i >> 3] &= (uint8_t)~mask;
        }
    }
}

// ---- P25p1 Golay(24,12,8)/(18,6,8) and Reed-Solomon GF(64) hard-decision decoders ----------------------------------
static int
rs_code_params(int code, int* n_par, int* n_data, int* t) {
    switch (code) {
        case DDN_RS_24_12_13: *n_par = 12; *n_data = 12; *t = 6; return DDN_OK;
        case DDN_RS_24_16_9: *n_par = 8; *n_data = 16; *t = 4; return DDN_OK;
        case DDN_RS_36_20_17: *n_par = 16; *n_data = 20; *t = 8; return DDN_OK;
        default: ddn_set_error("unknown RS code id %d", code); return DDN_EINVAL;
    }
}

static int
check_golay24(const char* who, int data_len, const uint8_t* data_bits, const uint8_t* parity12, const uint8_t* status) {
    return ((data_len == 6 || data_len == 12) && data_bits && parity12 && status) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_golay24_batch(int data_len, uint8_t* d_data_bits, const uint8_t* d_parity12, size_t n, uint8_t* d_status,
                      int32_t* d_fixed, void* hip_stream) {
    DDN_TRY(check_golay24(__func__, data_len, d_data_bits, d_parity12, d_status));
    HIP_TRY(ddn_dev_golay24(d_data_bits, d_parity12, data_len, (int)n, d_status, d_fixed, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_golay24_host(int data_len, uint8_t* data_bits, const uint8_t* parity12, size_t n, uint8_t* status,
                     int32_t* fixed) {
    DDN_TRY(check_golay24(__func__, data_len, data_bits, parity12, status));
    DdnStaged s;
    uint8_t* a = s.inout(data_bits, n * (size_t)data_len);
    const uint8_t* p = s.in(parity12, n * 12);
    uint8_t* st = s.out(status, n);
    int32_t* f = s.out(fixed, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_golay24_batch(data_len, a, p, n, st, f, nullptr));
    return s.finish();
}

static int
check_p25_rs(const char* who, int code, const uint8_t* data_bits, const uint8_t* parity_bits, const uint8_t* status, int* n_par, int* n_data,
             int* t) {
    DDN_TRY(rs_code_params(code, n_par, n_data, t));
    return (data_bits && parity_bits && status) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_p25_rs_batch(int code, uint8_t* d_data_bits, const uint8_t* d_parity_bits, size_t n, uint8_t* d_status,
                     void* hip_stream) {
    int n_par, n_data, t;
    DDN_TRY(check_p25_rs(__func__, code, d_data_bits, d_parity_bits, d_status, &n_par, &n_data, &t));
    HIP_TRY(ddn_dev_rs63(d_data_bits, d_parity_bits, n_par, n_data, t, (int)n, d_status, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_p25_rs_host(int code, uint8_t* data_bits, const uint8_t* parity_bits, size_t n, uint8_t* status) {
    int n_par, n_data, t;
    DDN_TRY(check_p25_rs(__func__, code, data_bits, parity_bits, status, &n_par, &n_data, &t));
    DdnStaged s;
    uint8_t* a = s.inout(data_bits, n * (size_t)n_data * 6);
    const uint8_t* p = s.in(parity_bits, n * (size_t)n_par * 6);
    uint8_t* st = s.out(status, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_p25_rs_batch(code, a, p, n, st, nullptr));
    return s.finish();
}

// reference names, one codeword per call (include/dsd-neo/protocol/p25/p25p1_check_hdu.h, p25p1_check_ldu.h).
// Return 1 ("irrecoverable") when the device path is unavailable, like the reference does when its decoder object
// could not be constructed (src/protocol/p25/phase1/p25p1_check_hdu.cpp:41-44).
static int
golay_one(int len, char* word, const char* parity, int* fixed_errors) {
    if (fixed_errors) {
        *fixed_errors = 0;
    }
    if (!fixed_errors || !word || !parity) {
        return 1;
    }
    uint8_t st = 1;
    int32_t fx = 0;
    if (ddn_fec_golay24_host(len, (uint8_t*)word, (const uint8_t*)parity, 1, &st, &fx) != DDN_OK) {
        return 1;
    }
    *fixed_errors = fx;
    return st;
}

extern "C" int
check_and_fix_golay_24_6(char* hex, const char* parity, int* fixed_errors) {
    return golay_one(6, hex, parity, fixed_errors);
}

extern "C" int
check_and_fix_golay_24_12(char* dodeca, const char* parity, int* fixed_errors) {
    return golay_one(12, dodeca, parity, fixed_errors);
}

static int
rs_one(int code, char* data, const char* parity) {
    uint8_t st = 1;
    if (!data || !parity || ddn_fec_p25_rs_host(code, (uint8_t*)data, (const uint8_t*)parity, 1, &st) != DDN_OK) {
        return 1;
    }
    return st;
}

extern "C" int
check_and_fix_reedsolomon_24_12_13(char* data, const char* parity) {
    return rs_one(DDN_RS_24_12_13, data, parity);
}

extern "C" int
check_and_fix_reedsolomon_24_16_9(char* data, const char* parity) {
    return rs_one(DDN_RS_24_16_9, data, parity);
}

extern "C" int
check_and_fix_redsolomon_36_20_17(char* data, const char* parity) {
    return rs_one(DDN_RS_36_20_17, data, parity);
}

// ---- P25 Phase 2 RS(63,35) sections (ESS / FACCH / SACCH) with caller-given erasures ------------------------------------
static int
rs28_sizes(int kind, int* n_data, int* n_par) {
    static const int nd[3] = {16, 26, 30}, np[3] = {28, 19, 22};
    if (kind < 0 || kind > 2) {
        ddn_set_error("rs28: kind must be DDN_RS28_ESS, _FACCH or _SACCH");
        return DDN_EINVAL;
    }
    *n_data = nd[kind];
    *n_par = np[kind];
    return DDN_OK;
}

static int
check_rs28(const char* who, int kind, const uint8_t* payload_bits, const uint8_t* parity_bits, const int8_t* erasures28,
           const uint8_t* n_erasures, const int32_t* status, int* n_data, int* n_par) {
    DDN_TRY(rs28_sizes(kind, n_data, n_par));
    return (payload_bits && parity_bits && status && (!n_erasures || erasures28)) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_rs28_batch(int kind, uint8_t* d_payload_bits, const uint8_t* d_parity_bits, const int8_t* d_erasures28,
                   const uint8_t* d_n_erasures, size_t n, int32_t* d_status, void* hip_stream) {
    int nd, np;
    DDN_TRY(check_rs28(__func__, kind, d_payload_bits, d_parity_bits, d_erasures28, d_n_erasures, d_status, &nd, &np));
    HIP_TRY(ddn_dev_rs28(kind, d_payload_bits, d_parity_bits, d_erasures28, d_n_erasures, (int)n, d_status,
                         (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_rs28_host(int kind, uint8_t* payload_bits, const uint8_t* parity_bits, const int8_t* erasures28,
                  const uint8_t* n_erasures, size_t n, int32_t* status) {
    int nd, np;
    DDN_TRY(check_rs28(__func__, kind, payload_bits, parity_bits, erasures28, n_erasures, status, &nd, &np));
    DdnStaged s;
    uint8_t* a = s.inout(payload_bits, n * (size_t)nd * 6);
    const uint8_t* p = s.in(parity_bits, n * (size_t)np * 6);
    const int8_t* e = s.in(erasures28, n * 28); // (a buffer also where no list is given)
    const uint8_t* c = s.in_opt(n_erasures, n);
    int32_t* st = s.out(status, n * sizeof(int32_t));
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_rs28_batch(kind, a, p, e, c, n, st, nullptr));
    return s.finish();
}

static int
check_xcch(const char* who, int kind, const uint8_t* bits360, const int16_t* llr360, const uint8_t* payload_bits, const int32_t* ec,
           const uint8_t* used_dynamic) {
    return ((kind == 0 || kind == 1) && bits360 && llr360 && payload_bits && ec && used_dynamic) ? DDN_OK : ddn_bad_argument(who);
}

// P25 Phase 2 FACCH / SACCH burst stage (include/ddn_hip.h): gather + ranked soft erasures + RS(63,35) with retries
extern "C" int
ddn_p25p2_xcch_batch(int kind, const uint8_t* d_bits360, const int16_t* d_llr360, size_t n, int threshold, uint8_t* d_payload_bits,
                     int32_t* d_ec, uint8_t* d_used_dynamic, void* hip_stream) {
    DDN_TRY(check_xcch(__func__, kind, d_bits360, d_llr360, d_payload_bits, d_ec, d_used_dynamic));
    if (n == 0) {
        return DDN_OK;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    DdnScratch s(st); // parity bits, erasure lists and their lengths
    const size_t n_pa = kind == 0 ? 114 : 132;
    uint8_t *parity, *n_total;
    int8_t* er;
    HIP_TRY(s.arena(n * (n_pa + 28 + 1) + 3 * 256));
    HIP_TRY(s.get(&parity, n * n_pa));
    HIP_TRY(s.get(&er, n * 28));
    HIP_TRY(s.get(&n_total, n));
    HIP_TRY(ddn_dev_p25p2_xcch(kind, d_bits360, d_llr360, (int)n, threshold, d_payload_bits, parity, er, n_total, d_ec, d_used_dynamic, st));
    return DDN_OK;
}

static int
check_mac_crc(const char* who, int kind, const uint8_t* payload_bits, const uint8_t* crc12_ok) {
    return ((kind == 0 || kind == 1) && payload_bits && crc12_ok) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_p25p2_mac_crc_batch(int kind, const uint8_t* d_payload_bits, size_t n, uint8_t* d_crc12_ok, uint8_t* d_crc16_ok, void* hip_stream) {
    DDN_TRY(check_mac_crc(__func__, kind, d_payload_bits, d_crc12_ok));
    HIP_TRY(ddn_dev_p25p2_mac_crc(kind, d_payload_bits, (int)n, d_crc12_ok, d_crc16_ok, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_p25p2_mac_crc_host(int kind, const uint8_t* payload_bits, size_t n, uint8_t* crc12_ok, uint8_t* crc16_ok) {
    DDN_TRY(check_mac_crc(__func__, kind, payload_bits, crc12_ok));
    DdnStaged s;
    const uint8_t* a = s.in(payload_bits, n * (kind == 0 ? 156 : 180));
    uint8_t* b = s.out(crc12_ok, n);
    uint8_t* c = crc16_ok ? s.out(crc16_ok, n) : nullptr;
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25p2_mac_crc_batch(kind, a, n, b, c, nullptr));
    return s.finish();
}

static int
check_ess(const char* who, const uint8_t* payload_bits96, const int16_t* payload_llr96, const uint8_t* parity_bits168, const int16_t* parity_llr168,
          const uint8_t* payload_out96, const int32_t* ec, const uint8_t* used_dynamic) {
    return (payload_bits96 && payload_llr96 && parity_bits168 && parity_llr168 && payload_out96 && ec && used_dynamic) ? DDN_OK : ddn_bad_argument(who);
}

// P25 Phase 2 ESS and voice bursts (include/ddn_hip.h)
extern "C" int
ddn_p25p2_ess_batch(const uint8_t* d_payload_bits96, const int16_t* d_payload_llr96, const uint8_t* d_parity_bits168,
                    const int16_t* d_parity_llr168, size_t n, int threshold, uint8_t* d_payload_out96, int32_t* d_ec, uint8_t* d_used_dynamic,
                    void* hip_stream) {
    DDN_TRY(check_ess(__func__, d_payload_bits96, d_payload_llr96, d_parity_bits168, d_parity_llr168, d_payload_out96, d_ec, d_used_dynamic));
    if (n == 0) {
        return DDN_OK;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    DdnScratch s(st); // erasure lists and their lengths
    int8_t* er;
    uint8_t* n_total;
    HIP_TRY(s.arena(n * 29 + 2 * 256));
    HIP_TRY(s.get(&er, n * 28));
    HIP_TRY(s.get(&n_total, n));
    HIP_TRY(ddn_dev_p25p2_ess(d_payload_bits96, d_payload_llr96, d_parity_bits168, d_parity_llr168, (int)n, threshold, d_payload_out96, er, n_total,
                              d_ec, d_used_dynamic, st));
    return DDN_OK;
}

extern "C" int
ddn_p25p2_ess_host(const uint8_t* payload_bits96, const int16_t* payload_llr96, const uint8_t* parity_bits168, const int16_t* parity_llr168,
                   size_t n, int threshold, uint8_t* payload_out96, int32_t* ec, uint8_t* used_dynamic) {
    DDN_TRY(check_ess(__func__, payload_bits96, payload_llr96, parity_bits168, parity_llr168, payload_out96, ec, used_dynamic));
    DdnStaged s;
    const uint8_t* a = s.in(payload_bits96, n * 96);
    const int16_t* al = s.in(payload_llr96, n * 96 * 2);
    const uint8_t* b = s.in(parity_bits168, n * 168);
    const int16_t* bl = s.in(parity_llr168, n * 168 * 2);
    uint8_t* o = s.out(payload_out96, n * 96);
    int32_t* e = s.out(ec, n * sizeof(int32_t));
    uint8_t* u = s.out(used_dynamic, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25p2_ess_batch(a, al, b, bl, n, threshold, o, e, u, nullptr));
    return s.finish();
}

extern "C" int
ddn_p25p2_voice_frames_batch(const uint8_t* d_xbits360, const int16_t* d_xllr360, size_t n, int frame_count, uint8_t* d_ambe_fr,
                             uint8_t* d_ambe_rel, void* hip_stream) {
    if (!d_xbits360 || !d_xllr360 || !d_ambe_fr || !d_ambe_rel || frame_count < 1 || frame_count > 4) {
        ddn_set_error("ddn_p25p2_voice_frames_batch: bad argument");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_p25p2_voice_unpack(d_xbits360, d_xllr360, (int)n, frame_count, d_ambe_fr, d_ambe_rel, (hipStream_t)hip_stream));
    return DDN_OK;
}

// P25 Phase 2 frame scrambler (include/ddn_hip.h)
extern "C" int
ddn_p25p2_scramble_bits_batch(const uint64_t* d_seed44, size_t n, size_t bit_count, uint8_t* d_out_bits, void* hip_stream) {
    if (!d_seed44 || !d_out_bits || bit_count > (1u << 20)) {
        ddn_set_error("ddn_p25p2_scramble_bits_batch: bad argument");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_p25p2_scramble_bits(d_seed44, (int)n, (int)bit_count, d_out_bits, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_p25p2_descramble_batch(const uint8_t* d_bits, const int16_t* d_llr, const uint8_t* d_scramble4320, const int32_t* d_offset,
                           const int32_t* d_sequence_of, size_t n, int n_bits, int n_llr, uint8_t* d_xbits, int16_t* d_xllr,
                           void* hip_stream) {
    if (!d_bits || !d_scramble4320 || !d_offset || !d_xbits || n_bits <= 0 || n_llr < 0 || n_llr > n_bits || (n_llr > 0 && (!d_llr || !d_xllr))) {
        ddn_set_error("ddn_p25p2_descramble_batch: bad argument");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_p25p2_descramble(d_bits, d_llr, d_scramble4320, d_offset, d_sequence_of, (int)n, n_bits, n_llr, d_xbits, d_xllr,
                                     (hipStream_t)hip_stream));
    return DDN_OK;
}

// the reference's name (src/protocol/p25/phase2/p25p2_frame_internal.h:28): one sequence, host pointers, staged through the device
extern "C" void
p25p2_generate_scramble_bits(uint64_t wacn, uint64_t sysid, uint64_t nac, uint8_t* out_bits, size_t bit_count) {
    if (!out_bits || bit_count == 0) {
        return;
    }
    const uint64_t seed = (wacn * 16777216ULL) + (sysid * 4096ULL) + nac;
    DdnStaged s;
    const uint64_t* a = s.in(&seed, 8);
    uint8_t* o = s.out(out_bits, bit_count);
    if (s.staged() == DDN_OK && ddn_p25p2_scramble_bits_batch(a, 1, bit_count, o, nullptr) == DDN_OK) {
        (void)s.finish(); // (the reference's function cannot fail: the error is in ddn_last_error())
    }
}

static int
check_burst_fields(const char* who, const uint8_t* bits360, const int16_t* llr360, const int32_t* duid, const int32_t* isch) {
    return (bits360 && llr360 && duid && isch) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_p25p2_burst_fields_batch(const uint8_t* d_bits360, const int16_t* d_llr360, size_t n, int threshold, int32_t* d_duid, int32_t* d_isch,
                             void* hip_stream) {
    DDN_TRY(check_burst_fields(__func__, d_bits360, d_llr360, d_duid, d_isch));
    if (n == 0) {
        return DDN_OK;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    DdnScratch s(st); // the I-ISCH words and their reliability rows
    uint64_t* words;
    uint8_t* rel;
    HIP_TRY(s.arena(n * 48 + 2 * 256));
    HIP_TRY(s.get(&words, n));
    HIP_TRY(s.get(&rel, n * 40));
    HIP_TRY(ddn_dev_p25p2_burst_fields(d_bits360, d_llr360, (int)n, threshold, d_duid, words, rel, st));
    HIP_TRY(ddn_dev_isch_lookup(words, rel, (int)n, d_isch, st));
    return DDN_OK;
}

extern "C" int
ddn_p25p2_burst_fields_host(const uint8_t* bits360, const int16_t* llr360, size_t n, int threshold, int32_t* duid, int32_t* isch) {
    DDN_TRY(check_burst_fields(__func__, bits360, llr360, duid, isch));
    DdnStaged s;
    const uint8_t* b = s.in(bits360, n * 360);
    const int16_t* l = s.in(llr360, n * 360 * 2);
    int32_t* d = s.out(duid, n * sizeof(int32_t));
    int32_t* q = s.out(isch, n * sizeof(int32_t));
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25p2_burst_fields_batch(b, l, n, threshold, d, q, nullptr));
    return s.finish();
}

extern "C" int
ddn_p25p2_xcch_host(int kind, const uint8_t* bits360, const int16_t* llr360, size_t n, int threshold, uint8_t* payload_bits, int32_t* ec,
                    uint8_t* used_dynamic) {
    DDN_TRY(check_xcch(__func__, kind, bits360, llr360, payload_bits, ec, used_dynamic));
    DdnStaged s;
    const uint8_t* b = s.in(bits360, n * 360);
    const int16_t* l = s.in(llr360, n * 360 * 2);
    uint8_t* p = s.out(payload_bits, n * (kind == 0 ? 156 : 180));
    int32_t* e = s.out(ec, n * sizeof(int32_t));
    uint8_t* u = s.out(used_dynamic, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25p2_xcch_batch(kind, b, l, n, threshold, p, e, u, nullptr));
    return s.finish();
}

// reference names (include/dsd-neo/fec/ez.h:29-31): one section per call, int-per-bit arrays.  -2 when the device path is
// unavailable, the value the reference returns when its decoder object could not be constructed (src/fec/ez.cpp:106-117).
static int
rs28_one(int kind, int* payload, const int* parity, const int* erasures, int n_erasures) {
    int nd, np;
    if (!payload || !parity || rs28_sizes(kind, &nd, &np) != DDN_OK) {
        return -2;
    }
    uint8_t pl[180], pa[168];
    int8_t er[28] = {0};
    for (int i = 0; i < nd * 6; i++) {
        pl[i] = (uint8_t)(payload[i] & 1);
    }
    for (int i = 0; i < np * 6; i++) {
        pa[i] = (uint8_t)(parity[i] & 1);
    }
    uint8_t ne = 0;
    for (int i = 0; erasures && i < n_erasures && i < 28; i++) {
        er[ne++] = (int8_t)erasures[i];
    }
    int32_t st = -2;
    if (ddn_fec_rs28_host(kind, pl, pa, er, &ne, 1, &st) != DDN_OK) {
        return -2;
    }
    for (int i = 0; i < nd * 6; i++) {
        payload[i] = pl[i];
    }
    return st;
}

extern "C" int
ez_rs28_ess(int payload[96], int parity[168], const int* erasures, int n_erasures) {
    return rs28_one(0, payload, parity, erasures, n_erasures);
}

extern "C" int
ez_rs28_facch(int payload[156], int parity[114], const int* erasures, int n_erasures) {
    return rs28_one(1, payload, parity, erasures, n_erasures);
}

extern "C" int
ez_rs28_sacch(int payload[180], int parity[132], const int* erasures, int n_erasures) {
    return rs28_one(2, payload, parity, erasures, n_erasures);
}

static int
check_isch_lookup(const char* who, const uint64_t* words, const int32_t* out) {
    return (words && out) ? DDN_OK : ddn_bad_argument(who);
}

// ---- P25 Phase 2 I-ISCH lookup ----------------------------------------------------------------------------------------------
extern "C" int
ddn_fec_isch_lookup_batch(const uint64_t* d_words, const uint8_t* d_reliab40, size_t n, int32_t* d_out, void* stream) {
    DDN_TRY(check_isch_lookup(__func__, d_words, d_out));
    HIP_TRY(ddn_dev_isch_lookup(d_words, d_reliab40, (int)n, d_out, (hipStream_t)stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_isch_lookup_host(const uint64_t* words, const uint8_t* reliab40, size_t n, int32_t* out) {
    DDN_TRY(check_isch_lookup(__func__, words, out));
    DdnStaged s;
    const uint64_t* w = s.in(words, n * sizeof(uint64_t));
    const uint8_t* r = s.in_opt(reliab40, n * 40);
    int32_t* o = s.out(out, n * sizeof(int32_t));
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_isch_lookup_batch(w, r, n, o, nullptr));
    return s.finish();
}

// reference names (include/dsd-neo/fec/ez.h): one word per call; -2 (the "nothing found" answer) when no device is there
extern "C" int
isch_lookup(uint64_t isch) {
    int32_t v = -2;
    return ddn_fec_isch_lookup_host(&isch, nullptr, 1, &v) == DDN_OK ? v : -2;
}

extern "C" int
isch_lookup_soft(uint64_t isch, const uint8_t reliab40[40]) {
    int32_t v = -2;
    return ddn_fec_isch_lookup_host(&isch, reliab40, 1, &v) == DDN_OK ? v : -2;
}

static int
check_soft_list(const char* who, const void* in, const void* candidates, const int32_t* counts, int max_candidates) {
    return (in && candidates && counts && max_candidates > 0) ? DDN_OK : ddn_bad_argument(who);
}

// ---- P25 1/2-rate list decoder -------------------------------------------------------------------------------------
extern "C" int
ddn_fec_p25_12_soft_list_batch(const int16_t* d_llr196, size_t n, int max_candidates, ddn_p25_12_candidate* d_candidates8,
                               int32_t* d_counts, void* hip_stream) {
    DDN_TRY(check_soft_list(__func__, d_llr196, d_candidates8, d_counts, max_candidates));
    HIP_TRY(ddn_dev_p25_half_rate_list(d_llr196, (int)n, max_candidates, (uint32_t*)d_candidates8, d_counts,
                                       (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_p25_12_soft_list_host(const int16_t* llr196, size_t n, int max_candidates, ddn_p25_12_candidate* candidates8,
                              int32_t* counts) {
    DDN_TRY(check_soft_list(__func__, llr196, candidates8, counts, max_candidates));
    DdnStaged s;
    const int16_t* a = s.in(llr196, n * 196 * 2);
    ddn_p25_12_candidate* c = s.out(candidates8, n * 8 * sizeof(ddn_p25_12_candidate));
    int32_t* k = s.out(counts, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_p25_12_soft_list_batch(a, n, max_candidates, c, k, nullptr));
    return s.finish();
}

// reference: int p25_12_soft_llr_list(const uint8_t* input, const int16_t* bit_llr196, p25_12_candidate_t* candidates,
//                                     int max_candidates)   (include/dsd-neo/protocol/p25/p25_12.h:31-32)
extern "C" int
p25_12_soft_llr_list(const uint8_t* input, const int16_t* bit_llr196, ddn_p25_12_candidate* candidates,
                     int max_candidates) {
    (void)input;
    if (!bit_llr196 || !candidates || max_candidates <= 0) {
        return 0;
    }
    ddn_p25_12_candidate tmp[8];
    int32_t cnt = 0;
    if (ddn_fec_p25_12_soft_list_host(bit_llr196, 1, max_candidates, tmp, &cnt) != DDN_OK) {
        return 0;
    }
    for (int i = 0; i < cnt; i++) {
        candidates[i] = tmp[i];
    }
    return cnt;
}

// ---- P25 confirmed data: rate 3/4 blocks on LLR pairs (p25p1_mbf34.c) --------------------------------------------------------
extern "C" int
ddn_fec_p25_mbf34_list_batch(const int16_t* d_llr196, size_t n, int max_candidates, const uint8_t* d_wanted,
                             ddn_p25_mbf34_candidate* d_candidates8, int32_t* d_counts, void* hip_stream) {
    DDN_TRY(check_soft_list(__func__, d_llr196, d_candidates8, d_counts, max_candidates));
    if (n == 0) {
        return DDN_OK;
    }
    HIP_TRY(ddn_dev_p25_mbf34_list(d_llr196, (int)n, max_candidates, d_wanted, (uint8_t*)d_candidates8, d_counts, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_p25_mbf34_list_host(const int16_t* llr196, size_t n, int max_candidates, ddn_p25_mbf34_candidate* candidates8, int32_t* counts) {
    DDN_TRY(check_soft_list(__func__, llr196, candidates8, counts, max_candidates));
    DdnStaged s;
    const int16_t* a = s.in(llr196, n * 196 * 2);
    ddn_p25_mbf34_candidate* c = s.out(candidates8, n * 8 * sizeof(ddn_p25_mbf34_candidate));
    int32_t* k = s.out(counts, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_p25_mbf34_list_batch(a, n, max_candidates, nullptr, c, k, nullptr));
    return s.finish();
}

// reference: p25_mbf34_decode_soft_list (include/dsd-neo/protocol/p25/p25p1_mbf34.h:28-29); dibits is unused there too
extern "C" int
p25_mbf34_decode_soft_list(const uint8_t dibits[98], const int16_t bit_llr[196], ddn_p25_mbf34_candidate* candidates, int max_candidates) {
    if (!dibits || !bit_llr || !candidates || max_candidates <= 0) {
        return 0;
    }
    ddn_p25_mbf34_candidate tmp[8];
    int32_t cnt = 0;
    if (ddn_fec_p25_mbf34_list_host(bit_llr, 1, max_candidates, tmp, &cnt) != DDN_OK) {
        return 0;
    }
    for (int i = 0; i < cnt; i++) {
        candidates[i] = tmp[i];
    }
    return cnt;
}

// ---- 3/4-rate list decoder -------------------------------------------------------------------------------------------
extern "C" int
ddn_fec_r34_list_batch(const uint8_t* d_dibits98, const uint8_t* d_reliab98, size_t n, int max_candidates,
                       ddn_r34_candidate* d_candidates32, int32_t* d_counts, void* hip_stream) {
    DDN_TRY(check_soft_list(__func__, d_dibits98, d_candidates32, d_counts, max_candidates));
    if (n == 0) {
        return DDN_OK;
    }
    // [n][49][8][32] back-pointer scratch, stream-ordered so concurrent calls never share it
    uint8_t* backs = nullptr;
    HIP_TRY(hipMallocAsync((void**)&backs, n * 49 * 8 * 32, (hipStream_t)hip_stream));
    const hipError_t e = ddn_dev_r34_list(d_dibits98, d_reliab98, (int)n, max_candidates, backs,
                                          (uint32_t*)d_candidates32, d_counts, (hipStream_t)hip_stream);
    HIP_TRY(hipFreeAsync(backs, (hipStream_t)hip_stream));
    HIP_TRY(e);
    return DDN_OK;
}

extern "C" int
ddn_fec_r34_list_host(const uint8_t* dibits98, const uint8_t* reliab98, size_t n, int max_candidates,
                      ddn_r34_candidate* candidates32, int32_t* counts) {
    DDN_TRY(check_soft_list(__func__, dibits98, candidates32, counts, max_candidates));
    DdnStaged s;
    const uint8_t* a = s.in(dibits98, n * 98);
    const uint8_t* r = s.in_opt(reliab98, n * 98);
    ddn_r34_candidate* c = s.out(candidates32, n * 32 * sizeof(ddn_r34_candidate));
    int32_t* k = s.out(counts, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_r34_list_batch(a, r, n, max_candidates, c, k, nullptr));
    return s.finish();
}

// reference: dmr_r34_viterbi_decode_list (include/dsd-neo/protocol/dmr/r34_viterbi.h:51-70)
extern "C" int
dmr_r34_viterbi_decode_list(const uint8_t* dibits98, const uint8_t* reliab98, ddn_r34_candidate* out_candidates,
                            int max_candidates, int* out_count) {
    if (!dibits98 || !out_candidates || !out_count || max_candidates <= 0) {
        return -1;
    }
    ddn_r34_candidate tmp[32];
    int32_t cnt = 0;
    if (ddn_fec_r34_list_host(dibits98, reliab98, 1, max_candidates, tmp, &cnt) != DDN_OK) {
        return -1;
    }
    for (int i = 0; i < cnt; i++) {
        out_candidates[i] = tmp[i];
    }
    *out_count = cnt;
    return 0;
}

static int
check_golay24_soft(const char* who, int data_len, const uint8_t* data_bits, const uint8_t* parity12, const int32_t* reliab, const uint8_t* status) {
    DDN_TRY(check_golay24(who, data_len, data_bits, parity12, status));
    return reliab ? DDN_OK : ddn_bad_argument(who);
}

// ---- soft (Chase) Golay / Hamming ------------------------------------------------------------------------------------
extern "C" int
ddn_fec_golay24_soft_batch(int data_len, uint8_t* d_data_bits, const uint8_t* d_parity12, const int32_t* d_reliab,
                           size_t n, uint8_t* d_status, int32_t* d_fixed, void* hip_stream) {
    DDN_TRY(check_golay24_soft(__func__, data_len, d_data_bits, d_parity12, d_reliab, d_status));
    HIP_TRY(ddn_dev_golay24_soft(d_data_bits, d_parity12, d_reliab, data_len, (int)n, d_status, d_fixed,
                                 (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_golay24_soft_host(int data_len, uint8_t* data_bits, const uint8_t* parity12, const int32_t* reliab, size_t n,
                          uint8_t* status, int32_t* fixed) {
    DDN_TRY(check_golay24_soft(__func__, data_len, data_bits, parity12, reliab, status));
    DdnStaged s;
    uint8_t* a = s.inout(data_bits, n * (size_t)data_len);
    const uint8_t* p = s.in(parity12, n * 12);
    const int32_t* r = s.in(reliab, n * (size_t)(data_len + 12) * 4);
    uint8_t* st = s.out(status, n);
    int32_t* f = s.out(fixed, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_golay24_soft_batch(data_len, a, p, r, n, st, f, nullptr));
    return s.finish();
}

static int
check_hamming_soft(const char* who, const uint8_t* bits10, const int32_t* reliab10, const uint8_t* out10, const uint8_t* status) {
    return (bits10 && reliab10 && out10 && status) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_hamming_10_6_3_soft_batch(const uint8_t* d_bits10, const int32_t* d_reliab10, size_t n, uint8_t* d_out10,
                                  uint8_t* d_status, void* hip_stream) {
    DDN_TRY(check_hamming_soft(__func__, d_bits10, d_reliab10, d_out10, d_status));
    HIP_TRY(ddn_dev_hamming_10_6_3_soft(d_bits10, d_reliab10, (int)n, d_out10, d_status, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_hamming_10_6_3_soft_host(const uint8_t* bits10, const int32_t* reliab10, size_t n, uint8_t* out10,
                                 uint8_t* status) {
    DDN_TRY(check_hamming_soft(__func__, bits10, reliab10, out10, status));
    DdnStaged s;
    const uint8_t* a = s.in(bits10, n * 10);
    const int32_t* r = s.in(reliab10, n * 40);
    uint8_t* o = s.out(out10, n * 10);
    uint8_t* st = s.out(status, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_hamming_10_6_3_soft_batch(a, r, n, o, st, nullptr));
    return s.finish();
}

// reference names (include/dsd-neo/protocol/p25/p25p1_soft.h): one codeword per call
static int
golay_soft_one(int len, char* data, const char* parity, const int* reliab, int* fixed) {
    if (!fixed) {
        return 1;
    }
    *fixed = 0;
    if (!data || !parity || !reliab) {
        return 1;
    }
    uint8_t st = 1;
    int32_t fx = 0;
    if (ddn_fec_golay24_soft_host(len, (uint8_t*)data, (const uint8_t*)parity, (const int32_t*)reliab, 1, &st, &fx)
        != DDN_OK) {
        return 1;
    }
    *fixed = fx;
    return st;
}

extern "C" int
check_and_fix_golay_24_6_soft(char* data, const char* parity, const int* reliab, int* fixed) {
    return golay_soft_one(6, data, parity, reliab, fixed);
}

extern "C" int
check_and_fix_golay_24_12_soft(char* data, const char* parity, const int* reliab, int* fixed) {
    return golay_soft_one(12, data, parity, reliab, fixed);
}

extern "C" int
hamming_10_6_3_soft(const char* bits, const int* reliab, char* out_bits) {
    if (!bits || !reliab || !out_bits) {
        return 2;
    }
    uint8_t st = 2;
    if (ddn_fec_hamming_10_6_3_soft_host((const uint8_t*)bits, (const int32_t*)reliab, 1, (uint8_t*)out_bits, &st)
        != DDN_OK) {
        memcpy(out_bits, bits, 10);
        return 2;
    }
    return st;
}

static int
check_p25_rs_soft(const char* who, int code, const uint8_t* data_bits, const uint8_t* parity_bits, const uint8_t* data_reliab,
                  const uint8_t* parity_reliab, const uint8_t* status, int* n_par, int* n_data, int* t) {
    DDN_TRY(check_p25_rs(who, code, data_bits, parity_bits, status, n_par, n_data, t));
    return (data_reliab && parity_reliab) ? DDN_OK : ddn_bad_argument(who);
}

// ---- RS with reliability-ranked erasures -------------------------------------------------------------------------------
extern "C" int
ddn_fec_p25_rs_soft_batch(int code, uint8_t* d_data_bits, const uint8_t* d_parity_bits, const uint8_t* d_data_reliab,
                          const uint8_t* d_parity_reliab, size_t n, uint8_t* d_status, void* hip_stream) {
    int n_par, n_data, t;
    DDN_TRY(check_p25_rs_soft(__func__, code, d_data_bits, d_parity_bits, d_data_reliab, d_parity_reliab, d_status, &n_par, &n_data, &t));
    HIP_TRY(ddn_dev_rs63_soft(d_data_bits, d_parity_bits, d_data_reliab, d_parity_reliab, n_par, n_data, t,
                              /*P25P1_SOFT_ERASURE_THRESHOLD*/ 64, (int)n, d_status, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_p25_rs_soft_host(int code, uint8_t* data_bits, const uint8_t* parity_bits, const uint8_t* data_reliab,
                         const uint8_t* parity_reliab, size_t n, uint8_t* status) {
    int n_par, n_data, t;
    DDN_TRY(check_p25_rs_soft(__func__, code, data_bits, parity_bits, data_reliab, parity_reliab, status, &n_par, &n_data, &t));
    DdnStaged s;
    uint8_t* a = s.inout(data_bits, n * (size_t)n_data * 6);
    const uint8_t* p = s.in(parity_bits, n * (size_t)n_par * 6);
    const uint8_t* dr = s.in(data_reliab, n * (size_t)n_data);
    const uint8_t* pr = s.in(parity_reliab, n * (size_t)n_par);
    uint8_t* st = s.out(status, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_p25_rs_soft_batch(code, a, p, dr, pr, n, st, nullptr));
    return s.finish();
}

static int
rs_soft_one(int code, char* data, const char* parity, const uint8_t* data_reliab, const uint8_t* parity_reliab) {
    uint8_t st = 1;
    if (!data || !parity || !data_reliab || !parity_reliab
        || ddn_fec_p25_rs_soft_host(code, (uint8_t*)data, (const uint8_t*)parity, data_reliab, parity_reliab, 1, &st)
               != DDN_OK) {
        return 1;
    }
    return st;
}

// reference names (include/dsd-neo/protocol/p25/p25p1_soft.h:90-110)
extern "C" int
p25p1_rs_24_12_13_soft_reliability(char* data, const char* parity, const uint8_t* data_reliab,
                                   const uint8_t* parity_reliab) {
    return rs_soft_one(DDN_RS_24_12_13, data, parity, data_reliab, parity_reliab);
}

extern "C" int
p25p1_rs_24_16_9_soft_reliability(char* data, const char* parity, const uint8_t* data_reliab,
                                  const uint8_t* parity_reliab) {
    return rs_soft_one(DDN_RS_24_16_9, data, parity, data_reliab, parity_reliab);
}

extern "C" int
p25p1_rs_36_20_17_soft_reliability(char* data, const char* parity, const uint8_t* data_reliab,
                                   const uint8_t* parity_reliab) {
    return rs_soft_one(DDN_RS_36_20_17, data, parity, data_reliab, parity_reliab);
}


static int
check_imbe_deinterleave(const char* who, const uint8_t* records10, const int64_t* first_record, const int32_t* status_count, const uint8_t* imbe_fr,
                        const uint8_t* imbe_soft, const uint8_t* flags, const int32_t* status_count_out) {
    return (records10 && first_record && status_count && imbe_fr && imbe_soft && flags && status_count_out) ? DDN_OK : ddn_bad_argument(who);
}

// ---- IMBE de-interleave (process_IMBE) ------------------------------------------------------------------------------
extern "C" int
ddn_p25p1_imbe_deinterleave_batch(const uint8_t* d_records10, size_t n_records, const int64_t* d_first_record,
                                  const int32_t* d_status_count, size_t n_frames, uint8_t* d_imbe_fr,
                                  uint8_t* d_imbe_soft, uint8_t* d_flags, int32_t* d_status_count_out,
                                  void* hip_stream) {
    DDN_TRY(check_imbe_deinterleave(__func__, d_records10, d_first_record, d_status_count, d_imbe_fr, d_imbe_soft, d_flags, d_status_count_out));
    HIP_TRY(ddn_dev_imbe_deinterleave(d_records10, (long)n_records, d_first_record, d_status_count, (int)n_frames,
                                      d_imbe_fr, d_imbe_soft, d_flags, d_status_count_out, (hipStream_t)hip_stream));
    return DDN_OK;
}

// internal (ddn_internal.h): the same over a live list of slots - the chain object's form
extern "C" int
ddn_p25p1_imbe_deinterleave_live(const uint8_t* d_records10, size_t n_records, const int64_t* d_first_record, const int32_t* d_status_count,
                                 size_t n_slots, const int32_t* d_live_slot, const int32_t* d_n_live, uint8_t* d_imbe_fr, uint8_t* d_imbe_soft,
                                 uint8_t* d_flags, int32_t* d_status_count_out, void* hip_stream) {
    DDN_TRY(check_imbe_deinterleave(__func__, d_records10, d_first_record, d_status_count, d_imbe_fr, d_imbe_soft, d_flags, d_status_count_out));
    if (!d_live_slot || !d_n_live || n_slots > (size_t)1 << 30) {
        return ddn_bad_argument(__func__);
    }
    HIP_TRY(ddn_dev_imbe_deinterleave_live(d_records10, (long)n_records, d_first_record, d_status_count, (int)n_slots, d_live_slot, d_n_live,
                                           d_imbe_fr, d_imbe_soft, d_flags, d_status_count_out, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_p25p1_imbe_deinterleave_host(const uint8_t* records10, size_t n_records, const int64_t* first_record,
                                 const int32_t* status_count, size_t n_frames, uint8_t* imbe_fr, uint8_t* imbe_soft,
                                 uint8_t* flags, int32_t* status_count_out) {
    DDN_TRY(check_imbe_deinterleave(__func__, records10, first_record, status_count, imbe_fr, imbe_soft, flags, status_count_out));
    DdnStaged s;
    const uint8_t* r = s.in(records10, n_records * 10);
    const int64_t* f = s.in(first_record, n_frames * 8);
    const int32_t* c = s.in(status_count, n_frames * 4);
    uint8_t* o = s.out(imbe_fr, n_frames * 184);
    uint8_t* so = s.out(imbe_soft, n_frames * 368);
    uint8_t* fl = s.out(flags, n_frames);
    int32_t* co = s.out(status_count_out, n_frames * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25p1_imbe_deinterleave_batch(r, n_records, f, c, n_frames, o, so, fl, co, nullptr));
    return s.finish();
}


static int
check_p25_lsd(const char* who, const uint8_t* bits16, const uint8_t* ok) {
    return (bits16 && ok) ? DDN_OK : ddn_bad_argument(who);
}

// ---- P25p1 low speed data (16,8) -----------------------------------------------------------------------------------------
extern "C" int
ddn_fec_p25_lsd_batch(uint8_t* d_bits16, const int16_t* d_llr16, size_t n, uint8_t* d_ok, void* hip_stream) {
    DDN_TRY(check_p25_lsd(__func__, d_bits16, d_ok));
    HIP_TRY(ddn_dev_p25_lsd(d_bits16, d_llr16, (int)n, d_ok, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_p25_lsd_host(uint8_t* bits16, const int16_t* llr16, size_t n, uint8_t* ok) {
    DDN_TRY(check_p25_lsd(__func__, bits16, ok));
    DdnStaged s;
    uint8_t* b = s.inout(bits16, n * 16);
    const int16_t* l = s.in_opt(llr16, n * 32);
    uint8_t* o = s.out(ok, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_p25_lsd_batch(b, l, n, o, nullptr));
    return s.finish();
}

// reference names (include/dsd-neo/protocol/p25/p25_lsd.h): 1 = valid or corrected, 0 = uncorrectable (also on failure)
extern "C" int
p25_lsd_fec_16x8(uint8_t* bits16) {
    uint8_t ok = 0;
    if (!bits16 || ddn_fec_p25_lsd_host(bits16, nullptr, 1, &ok) != DDN_OK) {
        return 0;
    }
    return ok;
}

extern "C" int
p25_lsd_fec_16x8_soft(uint8_t* bits16, const int16_t llr16[16]) {
    uint8_t ok = 0;
    if (!bits16 || ddn_fec_p25_lsd_host(bits16, llr16, 1, &ok) != DDN_OK) {
        return 0;
    }
    return ok;
}


static int
check_p25_crc16(const char* who, const uint8_t* bytes, int item_bytes, const uint8_t* ok) {
    return (bytes && ok && item_bytes >= 3) ? DDN_OK : ddn_bad_argument(who);
}

// ---- CRC-CCITT16 of decoded trunking blocks ---------------------------------------------------------------------------------
extern "C" int
ddn_fec_p25_crc16_batch(const uint8_t* d_bytes, int item_bytes, size_t n, uint8_t* d_ok, void* hip_stream) {
    DDN_TRY(check_p25_crc16(__func__, d_bytes, item_bytes, d_ok));
    HIP_TRY(ddn_dev_p25_crc16(d_bytes, item_bytes, (int)n, d_ok, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_p25_crc16_host(const uint8_t* bytes, int item_bytes, size_t n, uint8_t* ok) {
    DDN_TRY(check_p25_crc16(__func__, bytes, item_bytes, ok));
    DdnStaged s;
    const uint8_t* b = s.in(bytes, n * (size_t)item_bytes);
    uint8_t* o = s.out(ok, n);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_p25_crc16_batch(b, item_bytes, n, o, nullptr));
    return s.finish();
}

// reference name (include/dsd-neo/protocol/p25/p25_crc.h): payload = len + 16 ints holding one bit each; 0 good, 65535 bad
// (the reference's helper returns (uint16_t)-1 through an int)
extern "C" int
crc16_lb_bridge(const int* payload, int len) {
    if (!payload || len < 8 || (len & 7) || len + 16 > 190 * 1) {
        return 65535;
    }
    uint8_t bytes[32];
    const int nb = (len + 16) / 8;
    if (nb > (int)sizeof(bytes)) {
        return 65535;
    }
    for (int k = 0; k < nb; k++) {
        unsigned v = 0;
        for (int j = 0; j < 8; j++) {
            v = (v << 1) | (unsigned)(payload[8 * k + j] & 1);
        }
        bytes[k] = (uint8_t)v;
    }
    uint8_t ok = 0;
    if (ddn_fec_p25_crc16_host(bytes, nb, 1, &ok) != DDN_OK) {
        return 65535;
    }
    return ok ? 0 : 65535;
}
