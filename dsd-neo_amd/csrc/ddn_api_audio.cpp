// ddn_api_audio.cpp - C-ABI of the voice-frame auto gain (include/ddn_hip.h, kernel ddn_audio.hip)
#include <hip/hip_runtime.h>

#include "ddn_api_util.h"
#include "ddn_device.h"

static float
effective_gain(float audio_gain, int algid_0x21) { // agf_effective_gain(), src/core/audio/gain.c:47-58
    float gain = 1.0f;
    if (algid_0x21) {
        gain = 1.75f;
    }
    if (audio_gain != 0) {
        gain = audio_gain / 25.0f;
    }
    return gain;
}

static int
check_agf(const char* who, const float* pcm, int n_streams, int n_frames, const float* aout_gain) {
    return (pcm && aout_gain && n_streams > 0 && n_frames >= 0) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_audio_agf_batch(float* d_pcm, int n_streams, int n_frames, float audio_gain, int algid_0x21, float* d_aout_gain,
                    void* hip_stream) {
    DDN_TRY(check_agf(__func__, d_pcm, n_streams, n_frames, d_aout_gain));
    HIP_TRY(ddn_dev_agf(d_pcm, n_streams, n_frames, effective_gain(audio_gain, algid_0x21), d_aout_gain, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_audio_agf_host(float* pcm, int n_streams, int n_frames, float audio_gain, int algid_0x21, float* aout_gain) {
    DDN_TRY(check_agf(__func__, pcm, n_streams, n_frames, aout_gain));
    DdnStaged s;
    float* p = s.inout(pcm, (size_t)n_streams * (size_t)n_frames * 160 * 4);
    float* g = s.inout(aout_gain, (size_t)n_streams * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_audio_agf_batch(p, n_streams, n_frames, audio_gain, algid_0x21, g, nullptr));
    return s.finish();
}

// drop-in shape of agf() for one talk path: the caller's aout_gain travels as a plain float (the reference keeps it in dsd_state)
extern "C" int
ddn_agf_frame(float samp[160], float audio_gain, int algid_0x21, float* aout_gain_io) {
    return ddn_audio_agf_host(samp, 1, 1, audio_gain, algid_0x21, aout_gain_io);
}

// ---- the short-integer voice path (processAudio -> hpf_dL -> agsm) ----------------------------------------------------------
static float
hpf_d_coef() { // HPFilter_Init(&state->HRCFilterL, 960.0f, 1.0f / 8000.0f): src/core/util/dsd_misc.c:345-358,436-452
    float RC = 0.0;
    RC = 1.0 / (2 * 3.141592653 * 960.0f);
    return RC / ((1.0f / 8000.0f) + RC);
}

extern "C" int
ddn_audio_s16_state_init(float* state32, int n_streams) {
    if (!state32 || n_streams < 0) {
        return DDN_EINVAL;
    }
    for (int s = 0; s < n_streams; s++) {
        for (int i = 0; i < DDN_S16_STATE_FLOATS; i++) {
            state32[(size_t)s * DDN_S16_STATE_FLOATS + i] = 0.0f;
        }
        state32[(size_t)s * DDN_S16_STATE_FLOATS] = 25.0f; // state->aout_gain, src/core/util/dsd_init.c:580
    }
    return DDN_OK;
}

static int
check_s16(const char* who, const float* pcm, int n_streams, int n_frames, int use_agsm, const int16_t* out, const float* state32,
          const float* gain_a) {
    return (pcm && out && state32 && (!use_agsm || gain_a) && n_streams > 0 && n_frames >= 0) ? DDN_OK : ddn_bad_argument(who);
}

extern "C" int
ddn_audio_s16_batch(const float* d_pcm, int n_streams, int n_frames, float audio_gain, int use_hpf_d, int use_agsm,
                    int16_t* d_out, float* d_state32, float* d_gain_a, void* hip_stream) {
    DDN_TRY(check_s16(__func__, d_pcm, n_streams, n_frames, use_agsm, d_out, d_state32, d_gain_a));
    HIP_TRY(ddn_dev_audio_s16(d_pcm, n_streams, n_frames, audio_gain, use_hpf_d, use_agsm, hpf_d_coef(), d_out, d_state32,
                              d_gain_a, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_audio_s16_host(const float* pcm, int n_streams, int n_frames, float audio_gain, int use_hpf_d, int use_agsm, int16_t* out,
                   float* state32, float* gain_a) {
    DDN_TRY(check_s16(__func__, pcm, n_streams, n_frames, use_agsm, out, state32, gain_a));
    const size_t np = (size_t)n_streams * (size_t)n_frames * 160;
    DdnStaged s;
    const float* p = s.in(pcm, np * 4);
    int16_t* o = s.out(out, np * 2);
    float* st = s.inout(state32, (size_t)n_streams * DDN_S16_STATE_FLOATS * 4);
    float* g = s.inout(gain_a, (size_t)n_streams * 4); // (a buffer without the caller's too)
    DDN_TRY(s.staged());
    DDN_TRY(ddn_audio_s16_batch(p, n_streams, n_frames, audio_gain, use_hpf_d, use_agsm, o, st, g, nullptr));
    return s.finish();
}
