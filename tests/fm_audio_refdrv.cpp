// tests/fm_audio_refdrv.cpp - TEST INFRASTRUCTURE ONLY: our own driver around the compiled reference (oracle/_ref/libdsdneo_ref.so)
// for full_demod()'s audio-monitor output kind.  It restates no arithmetic: it owns a `struct demod_state`, sets the fields the way
// demod_init_common_defaults() does (src/io/radio/rtl_demod_config.cpp:258-337) plus the configuration under test, and calls the
// reference's public full_demod() on fixed blocks, like oracle/ref_harness.cpp does for the other two kinds.  Built at test time by
// tests/fm_audio.py where the reference's headers and the library exist; nothing compiled from it is kept in the repository.

#include <dsd-neo/dsp/demod_pipeline.h>
#include <dsd-neo/dsp/demod_state.h>
#include <dsd-neo/dsp/simd_widen.h>
#include <dsd-neo/runtime/mem.h>

#include <cstdint>
#include <cstring>
#include <new>

extern "C" {

// icfg: rate_out, profile, passes, post_downsample, deemph, (unused), audio_lpf_enable, dc_block, rate_in (what low_pass_real reads),
// rate_out2; fcfg: channel_squelch_level, squelch_env_attack, squelch_env_release (0 = the defaults), deemph_a, audio_lpf_alpha
void*
fmdrv_create(const int* icfg, const float* fcfg) {
    void* mem = dsd_neo_aligned_malloc(sizeof(demod_state));
    if (!mem) {
        return nullptr;
    }
    demod_state* d = new (mem) demod_state();
    d->rate_in = icfg[8];
    d->rate_out = icfg[0];
    d->downsample_passes = icfg[2];
    d->post_downsample = icfg[3] > 0 ? icfg[3] : 1;
    d->deemph = icfg[4];
    d->rate_out2 = icfg[9] > 0 ? icfg[9] : -1;
    d->mode_demod = &dsd_fm_demod;
    d->output_kind = DSD_DEMOD_OUTPUT_AUDIO_MONITOR;
    d->pre_j = d->pre_r = 0.0f;
    d->fm_demod_history_valid = 0;
    d->prev_lpr_index = 0;
    d->deemph_a = fcfg[3];
    d->deemph_avg = 0.0f;
    d->channel_lpf_enable = 1;
    d->channel_lpf_profile = icfg[1];
    d->channel_squelch_level = fcfg[0];
    d->audio_lpf_enable = icfg[6];
    d->audio_lpf_alpha = fcfg[4];
    d->audio_lpf_state = 0.0f;
    d->now_lpr = 0.0f;
    d->dc_block = icfg[7];
    d->dc_avg = 0.0f;
    d->post_polydecim_enabled = 0;
    d->post_polydecim_M = 1;
    d->squelch_gate_open = 1;
    d->squelch_env = 1.0f;
    d->squelch_env_attack = fcfg[1] > 0.0f ? fcfg[1] : 0.125f;
    d->squelch_env_release = fcfg[2] > 0.0f ? fcfg[2] : 0.03125f;
    d->lowpassed = d->input_cb_buf;
    d->lp_len = 0;
    return d;
}

void
fmdrv_destroy(void* h) {
    demod_state* d = static_cast<demod_state*>(h);
    if (!d) {
        return;
    }
    if (d->post_polydecim_taps) {
        dsd_neo_aligned_free(d->post_polydecim_taps);
    }
    if (d->post_polydecim_hist) {
        dsd_neo_aligned_free(d->post_polydecim_hist);
    }
    d->~demod_state();
    dsd_neo_aligned_free(d);
}

// fmt 0 = cu8 (the reference's own widening), 1 = cf32; blocks of block_len input samples, the last one short
long
fmdrv_run(void* h, int fmt, const void* iq, long n_complex, int block_len, float* out) {
    demod_state* d = static_cast<demod_state*>(h);
    long done = 0, written = 0;
    while (done < n_complex) {
        long n = n_complex - done;
        if (n > block_len) {
            n = block_len;
        }
        if (fmt == 0) {
            widen_u8_to_f32_bias127(static_cast<const uint8_t*>(iq) + 2 * done, d->input_cb_buf, (uint32_t)(2 * n));
        } else {
            std::memcpy(d->input_cb_buf, static_cast<const float*>(iq) + 2 * done, sizeof(float) * 2 * (size_t)n);
        }
        d->lowpassed = d->input_cb_buf;
        d->lp_len = (int)(2 * n);
        full_demod(d);
        std::memcpy(out + written, d->result, (size_t)d->result_len * sizeof(float));
        written += d->result_len;
        done += n;
    }
    return written;
}

// pre_r pre_j deemph_avg audio_lpf_state dc_avg now_lpr squelch_env gate
void
fmdrv_state(void* h, float out8[8]) {
    const demod_state* d = static_cast<const demod_state*>(h);
    out8[0] = d->pre_r;
    out8[1] = d->pre_j;
    out8[2] = d->deemph_avg;
    out8[3] = d->audio_lpf_state;
    out8[4] = d->dc_avg;
    out8[5] = d->now_lpr;
    out8[6] = d->squelch_env;
    out8[7] = (float)d->squelch_gate_open;
}

void
fmdrv_phases(void* h, int out2[2]) {
    const demod_state* d = static_cast<const demod_state*>(h);
    out2[0] = d->post_polydecim_phase;
    out2[1] = d->prev_lpr_index;
}

int
fmdrv_taps(void* h, float out16[16]) {
    const demod_state* d = static_cast<const demod_state*>(h);
    if (!d->post_polydecim_taps || d->post_polydecim_K != 16) {
        return 0;
    }
    std::memcpy(out16, d->post_polydecim_taps, sizeof(float) * 16);
    return 16;
}
}
