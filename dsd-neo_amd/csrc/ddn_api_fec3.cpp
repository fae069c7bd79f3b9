// ddn_api_fec3.cpp - C-ABI of the DMR / NXDN block codes (include/ddn_hip.h, "block codes downstream of the receive
// loop"): batched device-pointer calls, host-buffer variants and the drop-ins with the reference's names
// (include/dsd-neo/fec/block_codes.h:19-43, bptc.h:20-26, rs_12_9.h:38-42).

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ddn_api_util.h"
#include "ddn_device.h"
#include "ddn_fec3.h"

static int
code_shape(int code, int* n, int* k) {
    static const int N[] = {7, 12, 13, 15, 16, 20, 24, 16}, K[] = {4, 8, 9, 11, 11, 8, 12, 7};
    if (code < 0 || code > DDN_CODE_QR_16_7_6) {
        return DDN_EINVAL;
    }
    *n = N[code];
    *k = K[code];
    return DDN_OK;
}

static int
check_block_code(const char* who, int code, const uint8_t* bits, size_t n_items, int nb_codewords, int* n, int* k) {
    return (code_shape(code, n, k) == DDN_OK && nb_codewords >= 1 && (!n_items || bits)) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_block_code_batch(int code, uint8_t* d_bits, size_t n_items, int nb_codewords, uint8_t* d_decoded, uint8_t* d_ok,
                         void* hip_stream) {
    int n, k;
    DDN_TRY(check_block_code(__func__, code, d_bits, n_items, nb_codewords, &n, &k));
    DDN_TRY(ddn_have_device());
    const bool multi = code >= DDN_CODE_HAMMING_12_8 && code <= DDN_CODE_HAMMING_16_11_4;
    HIP_TRY(ddn_dev_block_code(code, d_bits, n_items, multi ? nb_codewords : 1, multi ? d_decoded : nullptr, d_ok,
                               (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_block_code_host(int code, uint8_t* bits, size_t n_items, int nb_codewords, uint8_t* decoded, uint8_t* ok) {
    int n, k;
    DDN_TRY(check_block_code(__func__, code, bits, n_items, nb_codewords, &n, &k));
    const bool multi = code >= DDN_CODE_HAMMING_12_8 && code <= DDN_CODE_HAMMING_16_11_4;
    const int nb = multi ? nb_codewords : 1;
    DdnStaged s;
    uint8_t* b = s.inout(bits, n_items * (size_t)n * (size_t)nb);
    uint8_t* d = (multi && decoded) ? s.out(decoded, n_items * (size_t)k * (size_t)nb) : nullptr;
    uint8_t* o = s.out(ok, n_items);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_block_code_batch(code, b, n_items, nb_codewords, d, o, nullptr));
    return s.finish();
}

// (the other pairs of this file: with items to decode, the input and the required output are there)
static int
check_in_out(const char* who, size_t n, const uint8_t* in, const uint8_t* out) {
    return (!n || (in && out)) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_fec_bptc_196x96_batch(const uint8_t* d_in196, int deinterleave, size_t n, uint8_t* d_out96, uint8_t* d_r3,
                          uint32_t* d_errs, void* hip_stream) {
    DDN_TRY(check_in_out(__func__, n, d_in196, d_out96));
    DDN_TRY(ddn_have_device());
    HIP_TRY(ddn_dev_bptc_196x96(d_in196, deinterleave, n, d_out96, d_r3, d_errs, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_bptc_196x96_host(const uint8_t* in196, int deinterleave, size_t n, uint8_t* out96, uint8_t* r3, uint32_t* errs) {
    DDN_TRY(check_in_out(__func__, n, in196, out96));
    DdnStaged s;
    const uint8_t* i = s.in(in196, n * 196);
    uint8_t* o = s.out(out96, n * 96);
    uint8_t* r = s.out(r3, n * 3);
    uint32_t* e = s.out(errs, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_bptc_196x96_batch(i, deinterleave, n, o, r, e, nullptr));
    return s.finish();
}

// BPTC 128x77 (kind 0: item 128 bytes -> 77) and reverse-channel BPTC 16x2 (kind 1 even / 2 odd parity: 32 -> 32)
static int
bptc_small(const char* who, int kind, const uint8_t* d_in, size_t n, uint8_t* d_out, uint32_t* d_errs, hipStream_t st) {
    DDN_TRY(check_in_out(who, n, d_in, d_out));
    hipError_t e = kind == 0 ? ddn_dev_bptc_128x77(d_in, n, d_out, d_errs, st) : ddn_dev_bptc_16x2(d_in, n, kind == 2, d_out, d_errs, st);
    if (e != hipSuccess) {
        ddn_set_error("bptc kernel launch failed: %s", hipGetErrorString(e));
        return DDN_EHIP;
    }
    return DDN_OK;
}

static int
bptc_small_host(const char* who, int kind, const uint8_t* in, size_t n, uint8_t* out, uint32_t* errs) {
    DDN_TRY(check_in_out(who, n, in, out));
    DdnStaged s;
    const uint8_t* i = s.in(in, n * (kind == 0 ? 128 : 32));
    uint8_t* o = s.out(out, n * (kind == 0 ? 77 : 32));
    uint32_t* e = s.out(errs, n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(bptc_small(who, kind, i, n, o, e, nullptr));
    return s.finish();
}

extern "C" int
ddn_fec_bptc_128x77_batch(const uint8_t* d_in128, size_t n, uint8_t* d_out77, uint32_t* d_errs, void* stream) {
    return bptc_small(__func__, 0, d_in128, n, d_out77, d_errs, (hipStream_t)stream);
}

extern "C" int
ddn_fec_bptc_128x77_host(const uint8_t* in128, size_t n, uint8_t* out77, uint32_t* errs) {
    return bptc_small_host(__func__, 0, in128, n, out77, errs);
}

extern "C" int
ddn_fec_bptc_16x2_batch(const uint8_t* d_in32, size_t n, int parity_odd, uint8_t* d_out32, uint32_t* d_errs, void* stream) {
    return bptc_small(__func__, parity_odd ? 2 : 1, d_in32, n, d_out32, d_errs, (hipStream_t)stream);
}

extern "C" int
ddn_fec_bptc_16x2_host(const uint8_t* in32, size_t n, int parity_odd, uint8_t* out32, uint32_t* errs) {
    return bptc_small_host(__func__, parity_odd ? 2 : 1, in32, n, out32, errs);
}

extern "C" uint32_t
BPTC_128x77_Extract_Data(uint8_t InputDataMatrix[8][16], uint8_t DMRDataExtracted[77]) {
    uint32_t errs = 0xFFFFFFFFu;
    if (!InputDataMatrix || !DMRDataExtracted
        || bptc_small_host(__func__, 0, &InputDataMatrix[0][0], 1, DMRDataExtracted, &errs) != DDN_OK) {
        return 0xFFFFFFFFu;
    }
    return errs;
}

extern "C" uint32_t
BPTC_16x2_Extract_Data(uint8_t InputInterleavedData[32], uint8_t DMRDataExtracted[32], uint32_t ParityCheckTypeOdd) {
    uint32_t errs = 0xFFFFFFFFu;
    if (!InputInterleavedData || !DMRDataExtracted
        || bptc_small_host(__func__, ParityCheckTypeOdd ? 2 : 1, InputInterleavedData, 1, DMRDataExtracted, &errs) != DDN_OK) {
        return 0xFFFFFFFFu;
    }
    return errs;
}

static int
check_trellis(const char* who, const uint8_t* source_bits, int source_stride, size_t n, int result_len, const uint8_t* result_bits,
              int result_stride) {
    DDN_TRY(check_in_out(who, n, source_bits, result_bits));
    if (result_len <= 0 || source_stride < 2 * result_len + 6 || result_stride < result_len) {
        ddn_set_error("%s: a row needs 2 * result_len + 6 source bits (the last bit looks 8 ahead)", who);
        return DDN_ERANGE;
    }
    return DDN_OK;
}

extern "C" int
ddn_fec_trellis_decode_batch(const uint8_t* d_source_bits, int source_stride, size_t n, int result_len, uint8_t* d_result_bits,
                             int result_stride, void* hip_stream) {
    DDN_TRY(check_trellis(__func__, d_source_bits, source_stride, n, result_len, d_result_bits, result_stride));
    DDN_TRY(ddn_have_device());
    HIP_TRY(ddn_dev_trellis_greedy(d_source_bits, source_stride, n, result_len, d_result_bits, result_stride, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_trellis_decode_host(const uint8_t* source_bits, int source_stride, size_t n, int result_len, uint8_t* result_bits,
                            int result_stride) {
    DDN_TRY(check_trellis(__func__, source_bits, source_stride, n, result_len, result_bits, result_stride));
    DdnStaged s;
    const uint8_t* i = s.in(source_bits, n * (size_t)source_stride);
    uint8_t* o = s.out(result_bits, n * (size_t)result_stride);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_trellis_decode_batch(i, source_stride, n, result_len, o, result_stride, nullptr));
    return s.finish();
}

// drop-in: include/dsd-neo/fec/trellis.h:22.  The reference reads source[2p .. 2p+7] for p < result_len, i.e. the caller's buffer
// holds 2 * result_len + 6 bits (its callers pass the zero-padded de-punctured field).
extern "C" void
trellis_decode(uint8_t result[], const uint8_t source[], int result_len) {
    if (!result || !source || result_len <= 0) {
        return;
    }
    (void)ddn_fec_trellis_decode_host(source, 2 * result_len + 6, 1, result_len, result, result_len);
}

extern "C" int
ddn_fec_rs_12_9_batch(uint8_t* d_codewords12, size_t n, uint8_t* d_result, uint8_t* d_errors_found, uint8_t* d_syndrome3,
                      void* hip_stream) {
    DDN_TRY(check_in_out(__func__, n, d_codewords12, d_result));
    DDN_TRY(ddn_have_device());
    HIP_TRY(ddn_dev_rs_12_9(d_codewords12, n, d_result, d_errors_found, d_syndrome3, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_fec_rs_12_9_host(uint8_t* codewords12, size_t n, uint8_t* result, uint8_t* errors_found, uint8_t* syndrome3) {
    DDN_TRY(check_in_out(__func__, n, codewords12, result));
    DdnStaged s;
    uint8_t* c = s.inout(codewords12, n * 12);
    uint8_t* r = s.out(result, n);
    uint8_t* f = s.out(errors_found, n);
    uint8_t* y = s.out(syndrome3, n * 3);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fec_rs_12_9_batch(c, n, r, f, y, nullptr));
    return s.finish();
}

// ---- the reference's names ---------------------------------------------------------------------------------------------
// The *_init() functions build file-static tables in the reference; here the tables are built with the library's first
// call on a device, so they are empty.
extern "C" void Hamming_7_4_init(void) {}
extern "C" void Hamming_12_8_init(void) {}
extern "C" void Hamming_13_9_init(void) {}
extern "C" void Hamming_15_11_init(void) {}
extern "C" void Hamming_16_11_4_init(void) {}
extern "C" void Golay_20_8_init(void) {}
extern "C" void Golay_24_12_init(void) {}
extern "C" void QR_16_7_6_init(void) {}
extern "C" void InitAllFecFunction(void) {}

static bool
one(int code, unsigned char* rx, unsigned char* dec, int nb) {
    uint8_t ok = 0;
    if (!rx || ddn_fec_block_code_host(code, rx, 1, nb, dec, &ok) != DDN_OK) {
        return false;
    }
    return ok != 0;
}

extern "C" bool Hamming_7_4_decode(unsigned char* rxBits) { return one(DDN_CODE_HAMMING_7_4, rxBits, nullptr, 1); }
extern "C" bool
Hamming_12_8_decode(unsigned char* rxBits, unsigned char* decodedBits, int nbCodewords) {
    return nbCodewords < 1 ? true : one(DDN_CODE_HAMMING_12_8, rxBits, decodedBits, nbCodewords);
}
extern "C" bool
Hamming_13_9_decode(unsigned char* rxBits, unsigned char* decodedBits, int nbCodewords) {
    return nbCodewords < 1 ? true : one(DDN_CODE_HAMMING_13_9, rxBits, decodedBits, nbCodewords);
}
extern "C" bool
Hamming_15_11_decode(unsigned char* rxBits, unsigned char* decodedBits, int nbCodewords) {
    return nbCodewords < 1 ? true : one(DDN_CODE_HAMMING_15_11, rxBits, decodedBits, nbCodewords);
}
extern "C" bool
Hamming_16_11_4_decode(unsigned char* rxBits, unsigned char* decodedBits, int nbCodewords) {
    return nbCodewords < 1 ? true : one(DDN_CODE_HAMMING_16_11_4, rxBits, decodedBits, nbCodewords);
}
extern "C" bool Golay_20_8_decode(unsigned char* rxBits) { return one(DDN_CODE_GOLAY_20_8, rxBits, nullptr, 1); }
extern "C" bool Golay_24_12_decode(unsigned char* rxBits) { return one(DDN_CODE_GOLAY_24_12, rxBits, nullptr, 1); }
extern "C" bool QR_16_7_6_decode(unsigned char* rxBits) { return one(DDN_CODE_QR_16_7_6, rxBits, nullptr, 1); }

extern "C" void
BPTCDeInterleaveDMRData(const uint8_t* Input, uint8_t* Output) { // pure index permutation: host (src/fec/bptc.c:27-46)
    if (!Input || !Output) {
        return;
    }
    for (uint32_t i = 0; i < 196; i++) {
        Output[(i * 13u) % 196u] = Input[i] & 1u; // BPTCDeInterleavingIndex[i] = 13 i mod 196
    }
}

extern "C" uint32_t
BPTC_196x96_Extract_Data(uint8_t InputDeInteleavedData[196], uint8_t DMRDataExtracted[96], uint8_t R[3]) {
    uint32_t errs = 0xFFFFFFFFu;
    uint8_t r3[3] = {0, 0, 0};
    if (!InputDeInteleavedData || !DMRDataExtracted
        || ddn_fec_bptc_196x96_host(InputDeInteleavedData, 0, 1, DMRDataExtracted, r3, &errs) != DDN_OK) {
        return 0xFFFFFFFFu;
    }
    if (R) {
        memcpy(R, r3, 3);
    }
    return errs;
}

extern "C" void
rs_12_9_calc_syndrome(const rs_12_9_codeword_t* codeword, rs_12_9_poly_t* syndrome) {
    if (!codeword || !syndrome) {
        return;
    }
    uint8_t cw[12], res = 0, syn[3] = {0, 0, 0};
    memcpy(cw, codeword->data, 12);
    memset(syndrome->data, 0, sizeof(syndrome->data));
    if (ddn_fec_rs_12_9_host(cw, 1, &res, nullptr, syn) == DDN_OK) {
        memcpy(syndrome->data, syn, 3);
    }
}

extern "C" uint8_t
rs_12_9_check_syndrome(const rs_12_9_poly_t* syndrome) {
    return (syndrome && (syndrome->data[0] | syndrome->data[1] | syndrome->data[2])) ? 1 : 0;
}

// `syndrome` must be the one rs_12_9_calc_syndrome returned for this code word (what every caller passes): the device
// kernel recomputes it
extern "C" rs_12_9_correct_errors_result_t
rs_12_9_correct_errors(rs_12_9_codeword_t* codeword, const rs_12_9_poly_t* syndrome, uint8_t* errors_found) {
    (void)syndrome;
    uint8_t res = RS_12_9_CORRECT_ERRORS_RESULT_ERRORS_CANT_BE_CORRECTED, found = 0;
    if (!codeword || ddn_fec_rs_12_9_host(codeword->data, 1, &res, &found, nullptr) != DDN_OK) {
        return RS_12_9_CORRECT_ERRORS_RESULT_ERRORS_CANT_BE_CORRECTED;
    }
    if (errors_found) {
        *errors_found = found;
    }
    return res;
}
