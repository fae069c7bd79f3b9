/* ddn_host_fm_audio.c - host side of the analog FM monitor (include/ddn_hip.h): coefficient design and the output-count rule.
 * No device work.
 *
 *   deemph_a          stream_open_apply_deemphasis_from_config, src/io/radio/rtl_sdr_fm.cpp:6198-6210 (Q15 rounding included)
 *   audio_lpf_alpha   stream_open_apply_audio_lpf_from_config, :6222-6237
 *   decimator taps    audio_polydecim_design_taps, src/dsp/demod_pipeline.cpp:339-359 (K = 16, Hamming window, fc = 0.45 / M)
 *   counts            audio_polydecim_process :412-439 and low_pass_real :597-621: both emit by integer phases alone
 */
#include <math.h>
#include <string.h>

#include "ddn_internal.h"

#define DDN_PI 3.14159265358979323846

/* sin(pi x) / (pi x), 1 at the origin (the reference's dsd_neo_sinc) */
static double
unit_sinc(double x) {
    const double arg = DDN_PI * x;
    return x == 0.0 ? 1.0 : sin(arg) / arg;
}

/* de-emphasis pole for time constant tau at rate fs, as a Q15 fraction: round-to-nearest of (1 - e^(-1 / (fs tau))) 2^15, kept inside
 * [1, 2^15 - 1], handed back as that many 32768ths */
static float
deemph_q15_fraction(double fs, double tau_s) {
    const double pole = exp(-1.0 / (fs * tau_s));
    long steps = lrint((1.0 - pole) * 32768.0);
    steps = steps < 1 ? 1 : (steps > 32767 ? 32767 : steps);
    return (float)((double)steps / 32768.0);
}

/* one-pole smoothing factor 1 - e^(-2 pi fc / fs), kept inside [0, 1] */
static float
one_pole_alpha(double fs, int cutoff_hz) {
    const double exponent = -2.0 * DDN_PI * (double)cutoff_hz / fs;
    return (float)fmin(fmax(1.0 - exp(exponent), 0.0), 1.0);
}

/* the post-demod decimator's low-pass: 16 points of a sinc of cut-off 0.45 / M cycles per sample centred on point 7, under a Hamming
 * window over points 0..15, scaled to unit sum.  Every product is formed once in binary64, summed in index order, and each tap is its
 * product over that sum, rounded to binary32. */
static void
decimator_taps(int M, float taps16[16]) {
    const double two_fc = 2.0 * (0.45 / (double)M);
    double weighted[16], total = 0.0;
    for (int i = 0; i < 16; i++) {
        const double hamming = 0.54 - 0.46 * cos(2.0 * DDN_PI * (double)i / 15.0);
        const double ideal = two_fc * unit_sinc(two_fc * (double)(i - 7));
        weighted[i] = ideal * hamming;
        total += weighted[i];
    }
    if (total == 0.0) {
        total = 1.0;
    }
    for (int i = 0; i < 16; i++) {
        taps16[i] = (float)(weighted[i] / total);
    }
}

static int
config_ok(const ddn_fm_audio_config* cfg) {
    const int tau = cfg->deemph_tau_us;
    if (tau != 0 && tau != 50 && tau != 75 && tau != 750) {
        ddn_set_error("ddn_fm_audio_config: deemph_tau_us %d is not 0 (75), 50, 75 or 750", tau);
        return DDN_EINVAL;
    }
    if (cfg->audio_lpf_cutoff_hz < 0 || !(cfg->squelch_env_attack >= 0.0f) || !(cfg->squelch_env_release >= 0.0f)) {
        ddn_set_error("ddn_fm_audio_config: negative audio_lpf_cutoff_hz or squelch envelope step");
        return DDN_EINVAL;
    }
    if (cfg->lpr_slow_hz > 0 && cfg->lpr_fast_hz < cfg->lpr_slow_hz) {
        ddn_set_error("ddn_fm_audio_config: lpr_slow_hz %d above lpr_fast_hz %d (the reference's prev_lpr_index grows without bound)",
                      cfg->lpr_slow_hz, cfg->lpr_fast_hz);
        return DDN_ERANGE;
    }
    return DDN_OK;
}

int
ddn_fm_audio_design(int rate_out_hz, const ddn_fm_audio_config* cfg, float out3[3], float taps16[16]) {
    if (!cfg || !out3 || !taps16) {
        ddn_set_error("ddn_fm_audio_design: null argument");
        return DDN_EINVAL;
    }
    const int rc = config_ok(cfg);
    if (rc != DDN_OK) {
        return rc;
    }
    const double fs = rate_out_hz < 1 ? 1.0 : (double)rate_out_hz;
    const double tau_s = cfg->deemph_tau_us == 50 ? 50e-6 : (cfg->deemph_tau_us == 750 ? 750e-6 : 75e-6);
    out3[0] = cfg->deemph ? deemph_q15_fraction(fs, tau_s) : 0.0f;
    out3[1] = cfg->audio_lpf_cutoff_hz > 0 ? one_pole_alpha(fs, cfg->audio_lpf_cutoff_hz < 100 ? 100 : cfg->audio_lpf_cutoff_hz) : 0.0f;
    out3[2] = 1.0f / (float)(1 << 11);
    memset(taps16, 0, sizeof(float) * 16);
    if (cfg->post_downsample > 1) {
        decimator_taps(cfg->post_downsample, taps16);
    }
    return DDN_OK;
}

int
ddn_fm_audio_plan(const ddn_fm_audio_config* cfg, int passes, int block_len, size_t n, int* poly_phase, int* lpr_index,
                  size_t* out_count) {
    if (!cfg || !poly_phase || !lpr_index || !out_count || passes < 0 || passes > 30 || block_len <= 0) {
        ddn_set_error("ddn_fm_audio_plan: bad argument");
        return DDN_EINVAL;
    }
    const int rc = config_ok(cfg);
    if (rc != DDN_OK) {
        return rc;
    }
    const size_t mask = ((size_t)1 << passes) - 1;
    if ((n & mask) != 0 || ((size_t)block_len & mask) != 0) {
        ddn_set_error("ddn_fm_audio_plan: n = %zu and block_len = %d must be multiples of %d with %d decimation passes", n, block_len,
                      1 << passes, passes);
        return DDN_ERANGE;
    }
    const int M = cfg->post_downsample > 1 ? cfg->post_downsample : 1;
    const size_t nd = n >> passes, bl = (size_t)block_len >> passes;
    const size_t tail = nd % bl;
    if (bl < (size_t)M || (tail != 0 && tail < (size_t)M)) {
        ddn_set_error("ddn_fm_audio_plan: a block of %zu samples is shorter than post_downsample = %d (the reference keeps such a block "
                      "un-decimated, which is not restated)", bl < (size_t)M ? bl : tail, M);
        return DDN_ERANGE;
    }
    const int lpr = cfg->lpr_slow_hz > 0;
    if ((M > 1 && (*poly_phase < 0 || *poly_phase >= M)) || (lpr && (*lpr_index < 0 || *lpr_index >= cfg->lpr_fast_hz))) {
        ddn_set_error("ddn_fm_audio_plan: carried phase out of range");
        return DDN_EINVAL;
    }
    unsigned long long dec = nd;
    if (M > 1) { /* one output each time the phase counter reaches M */
        const unsigned long long t = (unsigned long long)*poly_phase + nd;
        dec = t / (unsigned long long)M;
        *poly_phase = (int)(t % (unsigned long long)M);
    }
    unsigned long long out = dec;
    if (lpr) { /* slow <= fast: at most one output per input, the index stays below fast */
        const unsigned long long t = (unsigned long long)*lpr_index + dec * (unsigned long long)cfg->lpr_slow_hz;
        out = t / (unsigned long long)cfg->lpr_fast_hz;
        *lpr_index = (int)(t % (unsigned long long)cfg->lpr_fast_hz);
    }
    *out_count = (size_t)out;
    return DDN_OK;
}
