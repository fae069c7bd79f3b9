// ddn_api_ted.cpp — C-ABI of the batched Gardner timing-recovery stage (include/ddn_hip.h, "timing recovery").
// Batched analogue of op25_gardner_cc(struct demod_state*) (reference include/dsd-neo/dsp/costas.h): the carried
// ted_state_t of every channel lives on the device inside the ddn_ted_batch object.

#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "ddn_api_util.h"
#include "ddn_device.h"

struct ddn_ted_batch {
    int n_channels, sps, symbol_rate_hz;
    float ted_gain;
    long block_len; // 0: one reference call per ddn_gardner_run; else the reference's block size in samples
    DdnTedState* d_state;
    float* d_dl;
    int* d_count;
    DdnPool pool;
};

extern "C" int
ddn_ted_batch_create(int n_channels, int sps, int symbol_rate_hz, float ted_gain, ddn_ted_batch** out) {
    if (!out || n_channels <= 0 || sps < 2 || sps > 49) {
        ddn_set_error("ddn_ted_batch_create: bad argument (sps must be 2..49 for the %d-entry delay line)", DDN_TED_DL);
        return DDN_EINVAL;
    }
    DDN_TRY(ddn_have_device());
    ddn_ted_batch* b = new (std::nothrow) ddn_ted_batch();
    if (!b) {
        return DDN_ENOMEM;
    }
    memset(b, 0, sizeof(*b));
    b->n_channels = n_channels;
    b->sps = sps;
    b->symbol_rate_hz = symbol_rate_hz;
    b->ted_gain = ted_gain;
    const size_t B = (size_t)n_channels;
    if (!b->pool.alloc(&b->d_state, B) || !b->pool.alloc(&b->d_dl, DDN_TED_DL * 4 * B) || !b->pool.alloc(&b->d_count, B)) {
        ddn_set_error("ddn_ted_batch_create: device allocation failed");
        ddn_ted_batch_destroy(b);
        return DDN_ENOMEM;
    }
    *out = b;
    return DDN_OK;
}

extern "C" void
ddn_ted_batch_destroy(ddn_ted_batch* b) {
    if (!b) {
        return;
    }
    b->pool.release();
    delete b;
}

extern "C" int
ddn_ted_batch_reset(ddn_ted_batch* b, void* hip_stream) {
    if (!b) {
        return DDN_EINVAL;
    }
    const size_t B = (size_t)b->n_channels;
    HIP_TRY(hipMemsetAsync(b->d_state, 0, sizeof(DdnTedState) * B, (hipStream_t)hip_stream));
    HIP_TRY(hipMemsetAsync(b->d_dl, 0, sizeof(float) * DDN_TED_DL * 4 * B, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_ted_batch_set_block_len(ddn_ted_batch* b, size_t block_len) {
    if (!b || (block_len != 0 && block_len < 4)) {
        ddn_set_error("ddn_ted_batch_set_block_len: bad argument (block_len must be 0 or >= 4)");
        return DDN_EINVAL;
    }
    b->block_len = (long)block_len;
    return DDN_OK;
}

static int
check_gardner(const char* who, const ddn_ted_batch* b, const float* iq, const float* sym, bool count_ok) {
    return (b && iq && sym && count_ok) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_gardner_run(ddn_ted_batch* b, const float* d_iq, size_t n, float* d_sym, size_t sym_stride, int* d_sym_count,
                void* hip_stream) {
    DDN_TRY(check_gardner(__func__, b, d_iq, d_sym, true));
    HIP_TRY(ddn_dev_gardner(d_iq, (long)n, n, b->n_channels, b->sps, b->ted_gain, b->symbol_rate_hz, b->block_len,
                            b->d_state, b->d_dl, d_sym, sym_stride, d_sym_count ? d_sym_count : b->d_count,
                            (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_gardner_run_host(ddn_ted_batch* b, const float* iq, size_t n, float* sym, size_t sym_stride, int* sym_count) {
    DDN_TRY(check_gardner(__func__, b, iq, sym, sym_count != nullptr));
    const size_t B = (size_t)b->n_channels;
    DdnStaged s;
    const float* in = s.in(iq, B * n * 8);
    float* o = s.out(sym, B * sym_stride * 8);
    int* c = s.out(sym_count, B * sizeof(int));
    DDN_TRY(s.staged());
    DDN_TRY(ddn_gardner_run(b, in, n, o, sym_stride, c, nullptr));
    return s.finish();
}

extern "C" int
ddn_ted_batch_get_state(ddn_ted_batch* b, int channel, float out8[8]) {
    if (!b || !out8 || channel < 0 || channel >= b->n_channels) {
        return DDN_EINVAL;
    }
    DdnTedState s;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&s, b->d_state + channel, sizeof(s), hipMemcpyDeviceToHost));
    out8[0] = s.mu;
    out8[1] = s.omega;
    out8[2] = s.last_r;
    out8[3] = s.last_j;
    out8[4] = s.lock_accum;
    out8[5] = (float)s.lock_count;
    out8[6] = (float)s.dl_index;
    out8[7] = (float)s.twice_sps;
    return DDN_OK;
}
