// ddn_batch.h - the batched front end's object, shared by the translation units that serve its output kinds (ddn_api.cpp: FSK
// discriminator; ddn_api_fm_audio.cpp: analog FM monitor).  Host code only (not installed).
#ifndef DDN_BATCH_H
#define DDN_BATCH_H

#include <hip/hip_runtime.h>

#include "ddn_device.h"
#include "ddn_internal.h"

struct ddn_batch {
    ddn_front_end_config cfg;
    float taps[DDN_MAX_TAPS + 1];
    int taps_len;
    int center;
    int group; // channels per workgroup of the fused kernel (8 or 16; 0 = by batch size)
    float* d_taps;
    // segments (ddn_batch_set_segments): tap sets of the second and third run of the channel index, where those runs start
    int n_seg, seg_first[3];
    float taps_s[2][DDN_MAX_TAPS + 1];
    float* d_taps_s[2];
    ddn_f2* d_carry;      // [B][DDN_CARRY_LEN]
    DdnFskState* d_state; // [B]
    // host-call staging
    void* d_in;
    size_t in_cap;
    float* d_out;
    size_t out_cap;
    int timing;
    hipEvent_t ev[3];
    int ev_valid;
    // half-band decimation cascade in front of the channel LPF (0 = none)
    int passes;
    void* d_hbhist[DDN_MAX_HB_PASSES]; // [B][taps_len-1] complex per stage
    void* d_dec[2];                    // ping-pong decimated streams
    size_t dec_cap[2];
    // optional IQ conditioning (row a5): unfused route channel LPF -> k_iq_cond_disc
    DdnIqCondConfig iqc;
    DdnIqCondState* d_iqstate; // [B]
    void* d_lpf_hist;          // [B][taps_len - 1] complex
    void* d_lpf;               // [B][n] complex channel-LPF output
    size_t lpf_cap;
    // analog FM monitor (ddn_batch_set_audio_monitor, ddn_api_fm_audio.cpp): the third output kind of full_demod()
    int audio_on;
    ddn_fm_audio_config audio_cfg;
    float audio_coef[3];  // deemph_a, audio_lpf_alpha, 2^-11
    float audio_taps[16]; // the post-demod decimator's taps (M > 1)
    int audio_phase;      // post_polydecim_phase: carried on the host, the emit pattern depends on lengths alone
    int audio_lpr_index;  // prev_lpr_index
    DdnFmAudioState* d_audio_state; // [B]
    float* d_audio_ring;            // [B][16] the decimator's last 16 inputs, oldest first
};

// helpers of ddn_api.cpp the other output kinds use
int ddn_batch_grow(void** p, size_t* cap, size_t need);
int ddn_batch_check_cs16_aligned(const char* who, int input_format, const void* d_iq);
int ddn_batch_run_cascade(ddn_batch* b, const char* who, const void** d_iq, int* in_fmt, size_t* n, int* block_len, hipStream_t st);
int ddn_batch_grow_lpf(ddn_batch* b, size_t n, hipStream_t st);
// the adapter's way in: demod_state carries deemph_a / audio_lpf_alpha themselves, not what they were derived from (ddn_api_fm_audio.cpp)
int ddn_batch_override_audio_coefficients(ddn_batch* b, float deemph_a, float audio_lpf_alpha);

#endif
