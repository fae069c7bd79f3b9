/* tests/fm_audio_ref.c - CPU restatement of full_demod() for DSD_DEMOD_OUTPUT_AUDIO_MONITOR with mode_demod = dsd_fm_demod
 * (src/dsp/demod_pipeline.cpp:1330-1350), one channel.  TEST INFRASTRUCTURE: built at test time by tests/fm_audio.py against the
 * oracle's exported, already pinned helpers (widen, half-band cascade, channel LPF, mean power, phase delta); pinned itself to the
 * compiled reference by tests/test_fm_audio_oracle.py and to tests/golden/fm_audio_*.npz everywhere else.
 * Compile with -ffp-contract=off: the reference unit is built without FMA.
 *
 *   squelch gate                          full_demod_update_channel_state :1003-1020
 *   dsd_fm_demod                          :628-666
 *   post decimation                       full_demod_apply_post_audio_decimation :1259-1293, audio_polydecim_* :339-439
 *   deemph / audio LPF / DC block         :849-916
 *   low_pass_real                         :597-621
 *   squelch envelope                      full_demod_apply_squelch_envelope :1311-1325
 *   deemph_a, audio_lpf_alpha             src/io/radio/rtl_sdr_fm.cpp:6198-6210, :6222-6237
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ddn_oracle.h"

#define FMR_PI 3.14159265358979323846
#define FMR_K  16

typedef struct fmr {
    /* configuration */
    int rate_out, profile, passes, post_downsample, deemph, audio_lpf_enable, dc_block, lpr_fast, lpr_slow;
    float squelch_level, env_attack, env_release, deemph_a, audio_lpf_alpha;
    /* front of the path */
    float taps[ORC_MAX_TAPS];
    int taps_len;
    float hist_i[ORC_MAX_TAPS], hist_q[ORC_MAX_TAPS];
    float hb_hist_i[8][32], hb_hist_q[8][32];
    /* carried words of demod_state */
    float pre_r, pre_j;
    int history_valid;
    float ptaps[FMR_K];
    float recent[FMR_K]; /* the decimator's last 16 inputs, recent[0] the newest */
    int since_output;    /* inputs taken since the decimator's last output == the reference's phase counter */
    float deemph_avg, audio_lpf_state, dc_avg, now_lpr;
    int prev_lpr_index;
    float squelch_env;
    int gate_open;
} fmr;

size_t
fmr_sizeof(void) {
    return sizeof(fmr);
}

/* The decimator's 16 taps: Hamming-weighted samples of a sinc with cut-off 0.45 / M, centre at index 7, normalised to unit sum.
 * Same binary64 operations as the reference's designer; each weighted sample is formed once and kept. */
static void
fmr_decimator_taps(float* taps, int M) {
    const double pi = FMR_PI;
    const double scale = 2.0 * (0.45 / (double)M);
    double ws[FMR_K];
    double sum = 0.0;
    for (int j = 0; j < FMR_K; j++) {
        const double x = scale * (double)(j - (FMR_K - 1) / 2);
        const double lobe = (x == 0.0) ? 1.0 : sin(pi * x) / (pi * x);
        const double window = 0.54 - 0.46 * cos(2.0 * pi * (double)j / (double)(FMR_K - 1));
        ws[j] = (scale * lobe) * window;
        sum += ws[j];
    }
    const double norm = (sum == 0.0) ? 1.0 : sum;
    for (int j = 0; j < FMR_K; j++) {
        taps[j] = (float)(ws[j] / norm);
    }
}

/* icfg: rate_out, profile, passes, post_downsample, deemph, deemph_tau_us (0 = 75), audio_lpf_cutoff_hz (0 = off), dc_block,
 * lpr_fast, lpr_slow; fcfg: squelch_level, env_attack, env_release (0 = the defaults) */
int
fmr_init(fmr* s, const int* icfg, const float* fcfg) {
    memset(s, 0, sizeof(*s));
    s->rate_out = icfg[0];
    s->profile = icfg[1];
    s->passes = icfg[2];
    s->post_downsample = icfg[3];
    s->deemph = icfg[4];
    s->dc_block = icfg[7];
    s->lpr_fast = icfg[8];
    s->lpr_slow = icfg[9];
    s->squelch_level = fcfg[0];
    s->env_attack = fcfg[1];
    s->env_release = fcfg[2];
    s->taps_len = orc_channel_lpf_design(s->rate_out, s->profile, s->taps, ORC_MAX_TAPS);
    if (s->taps_len < 3 || s->passes > 8) {
        return -1;
    }
    const double rate = s->rate_out >= 1 ? (double)s->rate_out : 1.0;
    if (s->deemph) { /* 1 - e^(-1 / (rate tau)) in Q15, rounded to nearest, never 0 and never 1 */
        const double tau = icfg[5] == 50 ? 50e-6 : (icfg[5] == 750 ? 750e-6 : 75e-6);
        long q15 = lrint((1.0 - exp(-1.0 / (rate * tau))) * 32768.0);
        if (q15 > 32767) {
            q15 = 32767;
        }
        if (q15 < 1) {
            q15 = 1;
        }
        s->deemph_a = (float)((double)q15 / 32768.0);
    }
    if (icfg[6] > 0) { /* 1 - e^(-2 pi cutoff / rate), cutoff at least 100 Hz */
        const double cutoff = (double)(icfg[6] > 100 ? icfg[6] : 100);
        double g = 1.0 - exp(-2.0 * FMR_PI * cutoff / rate);
        g = g > 1.0 ? 1.0 : (g < 0.0 ? 0.0 : g);
        s->audio_lpf_alpha = (float)g;
        s->audio_lpf_enable = 1;
    }
    if (s->post_downsample > 1) {
        fmr_decimator_taps(s->ptaps, s->post_downsample);
    }
    s->squelch_env = 1.0f; /* demod_init_common_defaults */
    s->gate_open = 1;
    return s->taps_len;
}

void
fmr_set_coefficients(fmr* s, float deemph_a, float audio_lpf_alpha) {
    s->deemph_a = deemph_a;
    s->audio_lpf_alpha = audio_lpf_alpha;
}

void
fmr_get_coefficients(const fmr* s, float out3[3], float taps16[16]) {
    out3[0] = s->deemph_a;
    out3[1] = s->audio_lpf_alpha;
    out3[2] = 1.0f / (float)(1 << 11);
    memcpy(taps16, s->ptaps, sizeof(float) * FMR_K);
}

/* pre_r pre_j deemph_avg audio_lpf_state dc_avg now_lpr squelch_env gate */
void
fmr_get_state(const fmr* s, float out8[8]) {
    out8[0] = s->pre_r;
    out8[1] = s->pre_j;
    out8[2] = s->deemph_avg;
    out8[3] = s->audio_lpf_state;
    out8[4] = s->dc_avg;
    out8[5] = s->now_lpr;
    out8[6] = s->squelch_env;
    out8[7] = (float)s->gate_open;
}

void
fmr_get_phases(const fmr* s, int out2[2]) {
    out2[0] = s->since_output;
    out2[1] = s->prev_lpr_index;
}

static float
clampf(float v, float lo, float hi) {
    if (v < lo) {
        return lo;
    }
    if (v > hi) {
        return hi;
    }
    return v;
}

/* one full_demod() block of n_complex widened samples; scratch holds 6 * n_complex floats.  Returns result_len, or -1 where the
 * decimator yields nothing for the block (the reference then keeps the un-decimated block: not restated, refused by the library) */
static int
fmr_block(fmr* s, const float* iq, int n_complex, float* out, float* scratch) {
    float* a = scratch;
    float* b = scratch + 2 * (size_t)n_complex;
    float* res = scratch + 4 * (size_t)n_complex;
    float* tmp = scratch + 5 * (size_t)n_complex;
    const float* cur = iq;
    int len = 2 * n_complex;
    for (int i = 0; i < s->passes; i++) { /* full_demod_apply_halfband_decimation */
        float* dst = (cur == a) ? b : a;
        len = orc_hb_decim2_complex(cur, len, dst, s->hb_hist_i[i], s->hb_hist_q[i], i == 0 ? orc_hb31_taps : orc_hb15_taps,
                                    i == 0 ? 31 : 15, 1);
        cur = dst;
    }
    float* lp = (cur == a) ? b : a;
    if (len >= 2) {
        orc_fir_complex_apply(cur, len, lp, s->hist_i, s->hist_q, s->taps, s->taps_len, 1);
    }
    /* full_demod_update_channel_state */
    float pwr = 0.0f;
    if (len >= 2) {
        pwr = orc_mean_power(lp, len > 512 ? 512 : len, 1);
    }
    if (len > 0 && s->squelch_level > 0.0f && pwr < s->squelch_level) {
        s->gate_open = 0;
        for (int k = 0; k < len; k++) {
            lp[k] = 0.0f;
        }
    } else {
        s->gate_open = 1;
    }
    /* dsd_fm_demod */
    const int pairs = len >> 1;
    if (pairs <= 0) {
        return 0;
    }
    float prev_r = s->pre_r, prev_j = s->pre_j;
    if (!s->history_valid) {
        prev_r = lp[0];
        prev_j = lp[1];
        s->history_valid = 1;
    }
    for (int n = 0; n < pairs; n++) {
        const float cr = lp[2 * n], cj = lp[2 * n + 1];
        res[n] = orc_fsk_phase_delta(cr, cj, prev_r, prev_j);
        prev_r = cr;
        prev_j = cj;
    }
    s->pre_r = prev_r;
    s->pre_j = prev_j;
    int rl = pairs;
    /* post-demod decimation by M: every input enters the 16-deep history, every M-th one yields the dot of the history with the taps,
     * newest input against tap 0, accumulated from zero in that order */
    if (s->post_downsample > 1) {
        int made = 0;
        for (int n = 0; n < rl; n++) {
            memmove(s->recent + 1, s->recent, sizeof(float) * (FMR_K - 1));
            s->recent[0] = res[n];
            s->since_output++;
            if (s->since_output == s->post_downsample) {
                s->since_output = 0;
                float dot = 0.0f;
                for (int k = 0; k < FMR_K; k++) {
                    dot += s->recent[k] * s->ptaps[k];
                }
                tmp[made++] = dot;
            }
        }
        if (made == 0) {
            return -1;
        }
        memcpy(res, tmp, sizeof(float) * (size_t)made);
        rl = made;
    }
    /* full_demod_apply_audio_post_filters */
    if (s->deemph) {
        float avg = s->deemph_avg;
        const float alpha = clampf(s->deemph_a, 0.0f, 1.0f);
        for (int i = 0; i < rl; i++) {
            const float d = res[i] - avg;
            avg += d * alpha;
            res[i] = avg;
        }
        s->deemph_avg = avg;
    }
    if (s->audio_lpf_enable) {
        float y = s->audio_lpf_state;
        const float alpha = clampf(s->audio_lpf_alpha, 0.0f, 1.0f);
        for (int i = 0; i < rl; i++) {
            const float d = res[i] - y;
            y += d * alpha;
            res[i] = y;
        }
        s->audio_lpf_state = y;
    }
    if (s->dc_block) {
        float dc = s->dc_avg;
        const float k_scale = 1.0f / (float)(1 << 11);
        for (int i = 0; i < rl; i++) {
            const float x = res[i];
            dc += (x - dc) * k_scale;
            res[i] = x - dc;
        }
        s->dc_avg = dc;
    }
    if (s->lpr_slow > 0) { /* low_pass_real: integrate, and dump scaled by 1 / (fast / slow) (integer quotient) whenever the rate credit
                            * reaches `fast`; the outputs overwrite the front of the same array */
        const int quotient = s->lpr_fast / s->lpr_slow;
        const float scale = 1.0f / (float)(quotient >= 1 ? quotient : 1);
        int kept = 0;
        for (int i = 0; i < rl; i++) {
            s->now_lpr += res[i];
            s->prev_lpr_index += s->lpr_slow;
            if (s->prev_lpr_index >= s->lpr_fast) {
                s->prev_lpr_index -= s->lpr_fast;
                res[kept++] = s->now_lpr * scale;
                s->now_lpr = 0.0f;
            }
        }
        rl = kept;
    }
    /* full_demod_apply_squelch_envelope */
    {
        float env = s->squelch_env;
        const float target = s->gate_open ? 1.0f : 0.0f;
        const float alpha = s->gate_open ? (s->env_attack > 0.0f ? s->env_attack : 0.125f) : (s->env_release > 0.0f ? s->env_release : 0.03125f);
        env = clampf(env + alpha * (target - env), 0.0f, 1.0f);
        s->squelch_env = env;
        for (int k = 0; k < rl; k++) {
            out[k] = res[k] * env;
        }
    }
    return rl;
}

/* fmt 0 = cu8, 1 = cf32, 2 = cs16 (widened as (float)s * 2^-15); blocks of block_len input samples, the last one short.
 * Returns the samples written, -1 on a block the reference would pass through un-decimated. */
long
fmr_run(fmr* s, int fmt, const void* iq, long n_complex, int block_len, float* out) {
    float* wide = (float*)malloc(sizeof(float) * 2 * (size_t)block_len);
    float* scratch = (float*)malloc(sizeof(float) * 6 * (size_t)block_len + 64);
    long done = 0, w = 0;
    while (done < n_complex) {
        long n = n_complex - done;
        if (n > block_len) {
            n = block_len;
        }
        if (fmt == 0) {
            orc_widen_u8((const uint8_t*)iq + 2 * done, wide, (size_t)(2 * n));
        } else if (fmt == 2) {
            const int16_t* p = (const int16_t*)iq + 2 * done;
            for (long k = 0; k < 2 * n; k++) {
                wide[k] = (float)p[k] * (1.0f / 32768.0f);
            }
        } else {
            memcpy(wide, (const float*)iq + 2 * done, sizeof(float) * 2 * (size_t)n);
        }
        const int got = fmr_block(s, wide, (int)n, out + w, scratch);
        if (got < 0) {
            w = -1;
            break;
        }
        w += got;
        done += n;
    }
    free(wide);
    free(scratch);
    return w;
}
