// ddn_api_fm_audio.cpp - C-ABI of the analog FM monitor on a ddn_batch (include/ddn_hip.h): full_demod()'s output kind
// DSD_DEMOD_OUTPUT_AUDIO_MONITOR as half-band cascade -> channel LPF (complex result in HBM) -> k_fm_audio (ddn_fm_audio.hip).
// The coefficients and the count rule are host code (ddn_host_fm_audio.c); the two integer phases that decide how many samples a
// call produces stay on the host side of the batch, so a call returns its count without waiting for the device.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ddn_api_util.h"
#include "ddn_batch.h"
#include "ddn_device.h"

extern "C" int
ddn_batch_set_audio_monitor(ddn_batch* b, const ddn_fm_audio_config* cfg) {
    if (!b) {
        return ddn_bad_argument(__func__);
    }
    if (!cfg) {
        b->audio_on = 0;
        return ddn_batch_reset(b, nullptr);
    }
    if (b->n_seg > 0 || b->iqc.dc_enable || b->iqc.bal_enable) {
        ddn_set_error("ddn_batch_set_audio_monitor: the audio-monitor kind has no segmented form and no IQ conditioning stages; the "
                      "batch has %s set", b->n_seg > 0 ? "segments" : "IQ conditioning");
        return DDN_EINVAL;
    }
    float coef[3], taps[16];
    DDN_TRY(ddn_fm_audio_design(b->cfg.sample_rate_hz, cfg, coef, taps));
    if (cfg->post_downsample > 1 && (b->cfg.block_len >> b->passes) < cfg->post_downsample) {
        ddn_set_error("ddn_batch_set_audio_monitor: a block of %d samples is shorter than post_downsample = %d",
                      b->cfg.block_len >> b->passes, cfg->post_downsample);
        return DDN_ERANGE;
    }
    const size_t B = (size_t)b->cfg.n_channels;
    if (!b->d_audio_state) {
        if (hipMalloc(&b->d_audio_state, sizeof(DdnFmAudioState) * B) != hipSuccess
            || hipMalloc(&b->d_audio_ring, sizeof(float) * B * 16) != hipSuccess
            || (!b->d_lpf_hist && hipMalloc(&b->d_lpf_hist, sizeof(ddn_f2) * B * (size_t)(b->taps_len - 1)) != hipSuccess)) {
            (void)hipFree(b->d_audio_state);
            (void)hipFree(b->d_audio_ring);
            b->d_audio_state = nullptr;
            b->d_audio_ring = nullptr;
            ddn_set_error("ddn_batch_set_audio_monitor: device allocation failed");
            return DDN_ENOMEM;
        }
    }
    b->audio_cfg = *cfg;
    memcpy(b->audio_coef, coef, sizeof(coef));
    memcpy(b->audio_taps, taps, sizeof(taps));
    b->audio_on = 1;
    return ddn_batch_reset(b, nullptr);
}

extern "C" size_t
ddn_fm_audio_max_samples(const ddn_batch* b, size_t n) {
    if (!b || !b->audio_on) {
        return 0;
    }
    const ddn_fm_audio_config* c = &b->audio_cfg;
    unsigned long long v = n >> b->passes;
    if (c->post_downsample > 1) { // the phase counter one short of an output
        v = (v + (unsigned long long)c->post_downsample - 1) / (unsigned long long)c->post_downsample;
    }
    if (c->lpr_slow_hz > 0) {
        v = ((unsigned long long)c->lpr_fast_hz - 1 + v * (unsigned long long)c->lpr_slow_hz) / (unsigned long long)c->lpr_fast_hz;
    }
    return (size_t)v;
}

static int
check_audio_run(const char* who, const ddn_batch* b, const void* iq, const float* audio, const size_t* out_count) {
    if (!b || !iq || !audio || !out_count) {
        return ddn_bad_argument(who);
    }
    if (!b->audio_on) {
        ddn_set_error("%s: the batch is not set to the audio-monitor kind (ddn_batch_set_audio_monitor)", who);
        return DDN_EINVAL;
    }
    return DDN_OK;
}

extern "C" int
ddn_fm_audio_run(ddn_batch* b, const void* d_iq, size_t n, float* d_audio, size_t audio_stride, size_t* out_count, void* hip_stream) {
    DDN_TRY(check_audio_run(__func__, b, d_iq, d_audio, out_count));
    DDN_TRY(ddn_batch_check_cs16_aligned(__func__, b->cfg.input_format, d_iq));
    *out_count = 0;
    if (n == 0) {
        return DDN_OK;
    }
    const ddn_fm_audio_config* c = &b->audio_cfg;
    int phase = b->audio_phase, lpr_index = b->audio_lpr_index;
    size_t count = 0;
    DDN_TRY(ddn_fm_audio_plan(c, b->passes, b->cfg.block_len, n, &phase, &lpr_index, &count));
    if (audio_stride < count) {
        ddn_set_error("ddn_fm_audio_run: this call produces %zu samples per channel, audio_stride is %zu", count, audio_stride);
        return DDN_ERANGE;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int B = b->cfg.n_channels;
    int block_len = b->cfg.block_len;
    int in_fmt = b->cfg.input_format;
    DDN_TRY(ddn_batch_run_cascade(b, "ddn_fm_audio_run", &d_iq, &in_fmt, &n, &block_len, st));
    DDN_TRY(ddn_batch_grow_lpf(b, n, st));
    if (b->timing) {
        HIP_TRY(hipEventRecord(b->ev[0], st));
    }
    HIP_TRY(ddn_dev_channel_lpf_c2c(d_iq, in_fmt, (long)n, n, block_len, B, b->d_taps, b->taps_len, taps_have_zero(b->taps, b->taps_len),
                                    b->d_lpf_hist, b->d_lpf, n, st));
    if (b->timing) {
        HIP_TRY(hipEventRecord(b->ev[1], st));
    }
    DdnFmAudioArgs a;
    memset(&a, 0, sizeof(a));
    a.in = b->d_lpf;
    a.out = d_audio;
    a.state = b->d_audio_state;
    a.ring = b->d_audio_ring;
    a.stride = n;
    a.out_stride = audio_stride;
    a.n = (long)n;
    a.block_len = block_len;
    a.n_channels = B;
    a.squelch_on = b->cfg.squelch_level > 0.0f ? 1 : 0;
    a.squelch_level = b->cfg.squelch_level;
    a.M = c->post_downsample > 1 ? c->post_downsample : 1;
    a.phase0 = b->audio_phase;
    memcpy(a.taps, b->audio_taps, sizeof(a.taps));
    a.deemph_on = c->deemph ? 1 : 0;
    a.lpf_on = c->audio_lpf_cutoff_hz > 0 ? 1 : 0;
    a.dc_on = c->dc_block_off ? 0 : 1;
    a.deemph_a = b->audio_coef[0]; // (a Q15 fraction and a clamped double: both inside [0, 1], where the filters' own clamps leave them)
    a.lpf_alpha = b->audio_coef[1];
    a.dc_scale = b->audio_coef[2];
    a.lpr_on = c->lpr_slow_hz > 0 ? 1 : 0;
    a.lpr_fast = c->lpr_fast_hz;
    a.lpr_slow = c->lpr_slow_hz;
    a.lpr_index0 = b->audio_lpr_index;
    if (a.lpr_on) { // low_pass_real: 1 / (float)(fast / slow), the division in integers
        int decim = c->lpr_fast_hz / c->lpr_slow_hz;
        decim = decim < 1 ? 1 : decim;
        a.lpr_recip = 1.0f / (float)decim;
    }
    a.env_attack = c->squelch_env_attack > 0.0f ? c->squelch_env_attack : 0.125f;
    a.env_release = c->squelch_env_release > 0.0f ? c->squelch_env_release : 0.03125f;
    HIP_TRY(ddn_dev_fm_audio(&a, st));
    if (b->timing) {
        HIP_TRY(hipEventRecord(b->ev[2], st));
        b->ev_valid = 1;
    }
    b->audio_phase = phase;
    b->audio_lpr_index = lpr_index;
    *out_count = count;
    return DDN_OK;
}

extern "C" int
ddn_fm_audio_host_run(ddn_batch* b, const void* h_iq, size_t n, float* h_audio, size_t audio_stride, size_t* out_count) {
    DDN_TRY(check_audio_run(__func__, b, h_iq, h_audio, out_count));
    *out_count = 0;
    if (n == 0) {
        return DDN_OK;
    }
    const size_t B = (size_t)b->cfg.n_channels;
    const size_t in_bytes = B * n * ddn_input_format_bytes(b->cfg.input_format);
    const size_t out_bytes = B * audio_stride * sizeof(float);
    DDN_TRY(ddn_batch_grow(&b->d_in, &b->in_cap, in_bytes));
    DDN_TRY(ddn_batch_grow((void**)&b->d_out, &b->out_cap, out_bytes > 0 ? out_bytes : sizeof(float)));
    HIP_TRY(hipMemcpy(b->d_in, h_iq, in_bytes, hipMemcpyHostToDevice));
    DDN_TRY(ddn_fm_audio_run(b, b->d_in, n, b->d_out, audio_stride, out_count, nullptr));
    if (*out_count > 0) { // the written part of every row
        HIP_TRY(hipMemcpy2D(h_audio, audio_stride * sizeof(float), b->d_out, audio_stride * sizeof(float), *out_count * sizeof(float), B,
                            hipMemcpyDeviceToHost));
    } else {
        HIP_TRY(hipDeviceSynchronize());
    }
    return DDN_OK;
}

extern "C" int
ddn_batch_get_audio_coefficients(const ddn_batch* b, float out3[3], float taps16[16]) {
    if (!b || !out3 || !taps16 || !b->audio_on) {
        return ddn_bad_argument(__func__);
    }
    memcpy(out3, b->audio_coef, sizeof(float) * 3);
    memcpy(taps16, b->audio_taps, sizeof(float) * 16);
    return DDN_OK;
}

int
ddn_batch_override_audio_coefficients(ddn_batch* b, float deemph_a, float audio_lpf_alpha) {
    if (!b || !b->audio_on) {
        return ddn_bad_argument(__func__);
    }
    // deemph_filter / audio_lpf_filter clamp their coefficient to [0, 1] on every call
    b->audio_coef[0] = deemph_a < 0.0f ? 0.0f : (deemph_a > 1.0f ? 1.0f : deemph_a);
    b->audio_coef[1] = audio_lpf_alpha < 0.0f ? 0.0f : (audio_lpf_alpha > 1.0f ? 1.0f : audio_lpf_alpha);
    return DDN_OK;
}

extern "C" int
ddn_batch_get_audio_state(ddn_batch* b, int channel, float out8[8]) {
    if (!b || !out8 || !b->audio_on || channel < 0 || channel >= b->cfg.n_channels) {
        return ddn_bad_argument(__func__);
    }
    DdnFmAudioState s;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&s, b->d_audio_state + channel, sizeof(s), hipMemcpyDeviceToHost));
    out8[0] = s.pre_r;
    out8[1] = s.pre_j;
    out8[2] = s.deemph_avg;
    out8[3] = s.audio_lpf_state;
    out8[4] = s.dc_avg;
    out8[5] = s.now_lpr;
    out8[6] = s.initialised ? s.squelch_env : 1.0f; // a fresh stream: demod_init_common_defaults
    out8[7] = s.initialised ? (float)s.gate_open : 1.0f;
    return DDN_OK;
}
