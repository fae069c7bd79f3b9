// ddn_api_slicer.cpp — C-ABI of the batched P25p1 slicer / soft-decision stage and the P25 matched filter
// (include/ddn_hip.h).  The per-channel slicer words of dsd_state (center/umid/lmid/min/max, the 128-symbol window,
// the two 1024-deep extrema rings and their binary64 sums) live on the device inside the batch object.

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ddn_api_util.h"
#include "ddn_device.h"

struct ddn_slicer_batch {
    int n_channels, negative;
    DdnSlicerState* d_state;
    float *d_sbuf, *d_minring, *d_maxring, *d_fhist;
    DdnPool pool;
};

static int
slicer_fill(ddn_slicer_batch* b) {
    // reset exactly like symbol_reset_rtl_fsk_discriminator_slicer() (reference src/dsp/dsd_symbol.c:1306-1326)
    const size_t B = (size_t)b->n_channels;
    DdnSlicerState s;
    memset(&s, 0, sizeof(s));
    s.center = 0.0f;
    s.min = -30000.0f;
    s.max = 30000.0f;
    s.lmid = -20000.0f;
    s.umid = 20000.0f;
    std::vector<DdnSlicerState> hs(B, s);
    std::vector<float> mn(1024 * B, -30000.0f), mx(1024 * B, 30000.0f);
    if (hipMemcpy(b->d_state, hs.data(), sizeof(s) * B, hipMemcpyHostToDevice) != hipSuccess
        || hipMemcpy(b->d_minring, mn.data(), sizeof(float) * 1024 * B, hipMemcpyHostToDevice) != hipSuccess
        || hipMemcpy(b->d_maxring, mx.data(), sizeof(float) * 1024 * B, hipMemcpyHostToDevice) != hipSuccess
        || hipMemset(b->d_sbuf, 0, sizeof(float) * 128 * B) != hipSuccess
        || hipMemset(b->d_fhist, 0, sizeof(float) * 90 * B) != hipSuccess) {
        ddn_set_error("slicer state upload failed");
        return DDN_EHIP;
    }
    return DDN_OK;
}

extern "C" int
ddn_slicer_batch_create(int n_channels, int negative_polarity, ddn_slicer_batch** out) {
    if (!out || n_channels <= 0) {
        return DDN_EINVAL;
    }
    DDN_TRY(ddn_have_device());
    ddn_slicer_batch* b = new (std::nothrow) ddn_slicer_batch();
    if (!b) {
        return DDN_ENOMEM;
    }
    memset(b, 0, sizeof(*b));
    b->n_channels = n_channels;
    b->negative = negative_polarity ? 1 : 0;
    const size_t B = (size_t)n_channels;
    if (!b->pool.alloc(&b->d_state, B) || !b->pool.alloc(&b->d_sbuf, 128 * B) || !b->pool.alloc(&b->d_minring, 1024 * B)
        || !b->pool.alloc(&b->d_maxring, 1024 * B) || !b->pool.alloc(&b->d_fhist, 90 * B) || slicer_fill(b) != DDN_OK) {
        ddn_set_error("ddn_slicer_batch_create: device allocation failed");
        ddn_slicer_batch_destroy(b);
        return DDN_ENOMEM;
    }
    *out = b;
    return DDN_OK;
}

extern "C" void
ddn_slicer_batch_destroy(ddn_slicer_batch* b) {
    if (!b) {
        return;
    }
    b->pool.release();
    delete b;
}

extern "C" int
ddn_slicer_batch_reset(ddn_slicer_batch* b) {
    if (!b) {
        return DDN_EINVAL;
    }
    HIP_TRY(hipDeviceSynchronize());
    return slicer_fill(b);
}

static int
check_run(const char* who, const ddn_slicer_batch* b, const void* in, const void* out) {
    return (b && in && out) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_p25_slicer_run(ddn_slicer_batch* b, const float* d_symbols, size_t n, uint8_t* d_records10, void* hip_stream) {
    DDN_TRY(check_run(__func__, b, d_symbols, d_records10));
    // The sequential kernel (one lane per channel walking every symbol) remains for short calls; from a few hundred
    // symbols on the parallel decomposition (ddn_slicer_par.hip) wins.  DDN_SLICER_SEQ forces the sequential one (A/B).
    static const bool force_seq = DDN_EXP_ENV("DDN_SLICER_SEQ") != nullptr;
    if (n >= 256 && !force_seq) {
        DdnScratch s((hipStream_t)hip_stream);
        float* scratch;
        HIP_TRY(s.arena(sizeof(float) * 4 * n * (size_t)b->n_channels));
        HIP_TRY(s.get(&scratch, 4 * n * (size_t)b->n_channels));
        HIP_TRY(ddn_dev_p25_slicer_par(d_symbols, (long)n, n, b->n_channels, b->negative, b->d_state, b->d_sbuf, b->d_minring, b->d_maxring,
                                       scratch, d_records10, n * 10, (hipStream_t)hip_stream));
        return DDN_OK;
    }
    HIP_TRY(ddn_dev_p25_slicer(d_symbols, (long)n, n, b->n_channels, b->negative, b->d_state, b->d_sbuf, b->d_minring,
                               b->d_maxring, d_records10, n * 10, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_p25_slicer_run_host(ddn_slicer_batch* b, const float* symbols, size_t n, uint8_t* records10) {
    DDN_TRY(check_run(__func__, b, symbols, records10));
    const size_t B = (size_t)b->n_channels;
    DdnStaged s;
    const float* i = s.in(symbols, B * n * 4);
    uint8_t* o = s.out(records10, B * n * 10);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25_slicer_run(b, i, n, o, nullptr));
    return s.finish();
}

extern "C" int
ddn_slicer_batch_get_thresholds(ddn_slicer_batch* b, int channel, float out5[5]) {
    if (!b || !out5 || channel < 0 || channel >= b->n_channels) {
        return DDN_EINVAL;
    }
    DdnSlicerState s;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&s, b->d_state + channel, sizeof(s), hipMemcpyDeviceToHost));
    out5[0] = s.center;
    out5[1] = s.umid;
    out5[2] = s.lmid;
    out5[3] = s.max;
    out5[4] = s.min;
    return DDN_OK;
}

extern "C" int
ddn_p25_matched_filter_run(ddn_slicer_batch* b, const float* d_in, size_t n, float* d_out, void* hip_stream) {
    DDN_TRY(check_run(__func__, b, d_in, d_out));
    if (d_in == d_out) {
        ddn_set_error("ddn_p25_matched_filter_run: in-place operation is not supported");
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_p25_matched_filter(d_in, (long)n, n, b->n_channels, b->d_fhist, d_out, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_p25_matched_filter_run_host(ddn_slicer_batch* b, const float* in, size_t n, float* out) {
    DDN_TRY(check_run(__func__, b, in, out));
    const size_t B = (size_t)b->n_channels;
    DdnStaged s;
    const float* i = s.in(in, B * n * 4);
    float* o = s.out(out, B * n * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_p25_matched_filter_run(b, i, n, o, nullptr));
    return s.finish();
}
