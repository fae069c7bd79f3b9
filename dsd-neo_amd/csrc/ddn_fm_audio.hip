// ddn_fm_audio.hip — the analog FM monitor: full_demod()'s output kind DSD_DEMOD_OUTPUT_AUDIO_MONITOR behind the channel LPF.
//
// reference (src/dsp/demod_pipeline.cpp, per full_demod() block, after the channel LPF):
//   mean_power over the first <= 512 floats + squelch gate (I/Q zeroed, nothing reset)   :926-945,1003-1020
//   dsd_fm_demod: phase delta of neighbouring samples, seeded history, pre_r / pre_j     :628-666, :63-72
//   audio_polydecim_process: 16-tap polyphase decimator by post_downsample               :412-439, :369-384
//   deemph_filter / audio_lpf_filter / dc_block_filter: one-pole recurrences            :849-916
//   low_pass_real: integrate-and-dump to rate_out2                                       :597-621
//   full_demod_apply_squelch_envelope: one step per block, then a scale                  :1311-1325
//
// The route is the one of k_iq_cond_disc (ddn_iqcond.hip): the channel LPF result comes from HBM, 64 channels per workgroup,
// [64 channels][64 samples] tiles through LDS, double-buffered.  Only the one-pole filters, low_pass_real and the binary64 power
// sum are recurrences: they run on wave 0, one lane per channel.  A phase delta reads two neighbouring samples and a decimator
// output is a 16-term dot over the last 16 phase deltas, so both are done by the four staging waves (16 channel rows each, one
// lane per sample) on the way into LDS: the recurrence lane reads finished, already compacted decimator outputs.  The emit
// patterns of the decimator and of low_pass_real depend on integers alone, so every thread knows where a tile's outputs go.
//
// The gate of a block zeroes its I/Q from the first sample on and is decided by the first 256 complex samples.  Those are
// staged once more, as raw floats in power tiles of 32 samples, ahead of time: the steps run P(0) P(1) A(0) P(2) A(1) ..., P(b)
// the power tiles of block b, A(b) its audio tiles, so gate(b) stands in LDS a whole pass before the staging waves need it for
// A(b) (and gate(b - 1) for the first phase delta of block b).  A block is never walked twice, only its power window.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_atan2f.h"
#include "ddn_device.h"

namespace {
typedef ddn_f2 f2;
constexpr int TS = 64;   // samples of an audio tile
constexpr int PT = 32;   // complex samples of a power tile (64 floats)
constexpr int PW = 256;  // complex samples under the power window (512 floats)
constexpr int ROW = 129; // floats of an LDS row: inputs [0, 64), outputs [64, 128), one of padding
constexpr int HW = 16 + TS; // decimator history row: the 16 phase deltas before the tile, then the tile's
constexpr int NSTAGE = 4;
constexpr int RPW = 64 / NSTAGE; // channel rows per staging wave

struct Step {
    long blk;
    int pass, tile; // pass 0 = power tiles, 1 = audio tiles, 2 = a bubble (nothing to process: the gate settles)
};

__device__ __forceinline__ float
phase_delta(f2 cur, f2 prev) { // dsd_fm_demod's body, phase_delta_small_angle_or_atan2
    const float re = cur.x * prev.x + cur.y * prev.y;
    const float im = cur.y * prev.x - cur.x * prev.y;
    if (re > 1.0e-7f && fabsf(im) <= (0.35f * re)) {
        const float q = im / re;
        const float q2 = q * q;
        return q * (1.0f + q2 * (-0.3333333333333333f + q2 * 0.2f));
    }
    return ddn_atan2f_fast(im, re);
}

__device__ __forceinline__ void
lds_wave_sync() { // LDS writes of this wave before, LDS reads of this wave after
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(64 * (1 + NSTAGE)) void
k_fm_audio(const DdnFmAudioArgs a) {
    extern __shared__ unsigned char smem_raw[];
    float(*tile)[64][ROW] = reinterpret_cast<float(*)[64][ROW]>(smem_raw);                                       // [2]
    float(*hist)[64][HW] = reinterpret_cast<float(*)[64][HW]>(smem_raw + sizeof(float) * 2 * 64 * ROW);         // [2]
    int(*gate_l)[64] = reinterpret_cast<int(*)[64]>(smem_raw + sizeof(float) * 2 * 64 * (ROW + HW));            // [4]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const bool stager = wave > 0;
    const int row0 = (wave - 1) * RPW;
    const int ch0 = blockIdx.x * 64;
    const int ch = ch0 + lane;
    const bool live = !stager && ch < a.n_channels;
    const f2* __restrict__ in = (const f2*)a.in;
    const long n = a.n;
    const int block_len = a.block_len;
    const long n_blocks = (n + block_len - 1) / block_len;
    const int M = a.M;

    auto blk_len = [&](long b) { return (int)((n - b * block_len) < block_len ? (n - b * block_len) : block_len); };
    auto tiles_of = [&](const Step& s) {
        const int bl = blk_len(s.blk);
        return s.pass == 0 ? ((bl < PW ? bl : PW) + PT - 1) / PT : (s.pass == 1 ? (bl + TS - 1) / TS : 1);
    };
    auto advance = [&](Step& s) { // the next step; false past the end
        if (++s.tile < tiles_of(s)) {
            return true;
        }
        s.tile = 0;
        if (!a.squelch_on) {
            return ++s.blk < n_blocks;
        }
        if (s.pass == 0) {
            if (s.blk == 0) { // P(0) -> P(1), or a bubble in front of A(0) where there is no second block
                if (n_blocks > 1) {
                    s.blk = 1;
                } else {
                    s.pass = 2;
                }
            } else {          // P(k) -> A(k - 1)
                s.blk -= 1;
                s.pass = 1;
            }
            return true;
        }
        if (s.pass == 2) {
            s.pass = 1;
            return true;
        }
        if (s.blk + 2 < n_blocks) { // A(b) -> P(b + 2)
            s.blk += 2;
            s.pass = 0;
            return true;
        }
        return ++s.blk < n_blocks;  // A(b) -> A(b + 1): the last block's gate is known already
    };
    // outputs of the decimator / of the whole chain after i samples of this call
    auto dec_upto = [&](long i) { return M > 1 ? (long)(((unsigned long long)a.phase0 + (unsigned long long)i) / (unsigned)M) : i; };
    auto out_upto = [&](long i) {
        const long d = dec_upto(i);
        return a.lpr_on ? (long)(((unsigned long long)a.lpr_index0 + (unsigned long long)d * (unsigned)a.lpr_slow) / (unsigned)a.lpr_fast) : d;
    };
    auto gate_of = [&](long b, int c) { return a.squelch_on ? gate_l[b & 3][c] != 0 : true; };

    int hp = 0; // staging waves: which half of hist holds the 16 phase deltas before the next audio tile
    auto stage = [&](const Step& s, int buf) {
        if (s.pass == 2) {
            return;
        }
        const int bl = blk_len(s.blk);
        if (s.pass == 0) { // raw floats of the power window, 64 per row
            const int wf = 2 * (bl < PW ? bl : PW) - s.tile * 2 * PT; // floats left in the window
            const float* inf = (const float*)a.in;
#pragma unroll
            for (int r = 0; r < RPW; r++) {
                const int c = row0 + r;
                float v = 0.0f;
                if (ch0 + c < a.n_channels && lane < wf) {
                    v = inf[2 * ((size_t)(ch0 + c) * a.stride + (size_t)(s.blk * block_len) + (size_t)s.tile * PT) + lane];
                }
                tile[buf][c][lane] = v;
            }
            return;
        }
        const long g0 = s.blk * block_len + (long)s.tile * TS;
        const int tn = (bl - s.tile * TS) < TS ? (bl - s.tile * TS) : TS;
        const f2 z = {0.0f, 0.0f};
        int first = 0, cnt = tn;
        if (M > 1) {
            first = M - 1 - (int)(((unsigned long long)a.phase0 + (unsigned long long)g0) % (unsigned)M);
            cnt = tn > first ? (tn - first + M - 1) / M : 0;
        }
        // four rows at a time: their loads in flight together, then their phase deltas
#pragma unroll 1
        for (int r0 = 0; r0 < RPW; r0 += 4) {
            f2 cur[4], p0[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int c = row0 + r0 + r;
                const bool ok = ch0 + c < a.n_channels;
                const bool open = gate_of(s.blk, c);
                const size_t base = (size_t)(ch0 + c) * a.stride;
                cur[r] = (ok && open && lane < tn) ? in[base + g0 + lane] : z;
                p0[r] = z;
                if (lane == 0 && ok) { // the sample before the tile's first
                    if (s.tile > 0) {
                        p0[r] = open ? in[base + g0 - 1] : z;
                    } else if (s.blk > 0) {
                        p0[r] = gate_of(s.blk - 1, c) ? in[base + g0 - 1] : z; // pre_r / pre_j: zero behind a closed block
                    } else {
                        const DdnFmAudioState st = a.state[ch0 + c];
                        const f2 pre = {st.pre_r, st.pre_j};
                        p0[r] = st.history_valid ? pre : cur[r]; // seeded from the stream's own first sample
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int c = row0 + r0 + r;
                f2 prev;
                prev.x = __shfl_up(cur[r].x, 1);
                prev.y = __shfl_up(cur[r].y, 1);
                if (lane == 0) {
                    prev = p0[r];
                }
                const float ang = phase_delta(cur[r], prev);
                if (M <= 1) {
                    tile[buf][c][lane] = ang;
                } else if (lane < tn) {
                    hist[hp][c][16 + lane] = ang;
                }
            }
        }
        if (M <= 1) {
            return;
        }
        lds_wave_sync();
#pragma unroll 2
        for (int r = 0; r < RPW; r++) {
            const int c = row0 + r;
            if (lane < cnt) { // audio_polydecim_dot_latest: newest first, acc += hist * tap
                const int i = 16 + first + lane * M;
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    acc += hist[hp][c][i - k] * a.taps[k];
                }
                tile[buf][c][lane] = acc;
            }
            if (lane < 16) { // the 16 newest become the next tile's carried ones (other half: no lane overwrites what another reads)
                hist[hp ^ 1][c][lane] = hist[hp][c][tn + lane];
            }
        }
        hp ^= 1;
    };
    auto flush = [&](const Step& s, int buf) { // outputs of a finished audio step -> HBM, compacted rows
        if (s.pass != 1) {
            return;
        }
        const long g0 = s.blk * block_len + (long)s.tile * TS;
        const int bl = blk_len(s.blk);
        const int tn = (bl - s.tile * TS) < TS ? (bl - s.tile * TS) : TS;
        const long o0 = out_upto(g0);
        const int oc = (int)(out_upto(g0 + tn) - o0);
#pragma unroll
        for (int r = 0; r < RPW; r++) {
            const int c = row0 + r;
            if (ch0 + c < a.n_channels && lane < oc) {
                a.out[(size_t)(ch0 + c) * a.out_stride + (size_t)o0 + lane] = tile[buf][c][64 + lane];
            }
        }
    };

    DdnFmAudioState st = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0, 1, 0};
    if (live) {
        st = a.state[ch];
        if (!st.initialised) { // demod_init_common_defaults: squelch_env = 1, gate open
            st.squelch_env = 1.0f;
            st.gate_open = 1;
            st.initialised = 1;
        }
    }
    if (stager && M > 1) { // the decimator's ring as it stood before this call
        for (int r = 0; r < RPW; r++) {
            const int c = row0 + r;
            if (lane < 16) {
                hist[0][c][lane] = ch0 + c < a.n_channels ? a.ring[(size_t)(ch0 + c) * 16 + lane] : 0.0f;
            }
        }
    }
    Step cur = {0, a.squelch_on ? 0 : 1, 0};
    Step prev = cur;
    bool have_prev_step = false;
    if (stager && n > 0) {
        stage(cur, 0);
    }
    __syncthreads();
    double pw_t = 0.0, pw_p = 0.0;
    int lpr_index = a.lpr_index0;
    int buf = 0;
    bool more = n > 0;
    while (more) {
        Step nxt = cur;
        const bool has_next = advance(nxt);
        if (stager) {
            if (has_next) {
                stage(nxt, buf ^ 1);
            }
            if (have_prev_step) {
                flush(prev, buf ^ 1);
            }
        } else if (live) {
            const int bl = blk_len(cur.blk);
            if (cur.pass == 0) { // mean_power: t += s, p += s * s over the window's floats in order
                if (cur.tile == 0) {
                    pw_t = pw_p = 0.0;
                }
                const int len = 2 * (bl < PW ? bl : PW);
                const int wf = len - cur.tile * 2 * PT;
                const int tf = wf < 2 * PT ? wf : 2 * PT;
                for (int j = 0; j < tf; j++) {
                    const double s = (double)tile[buf][lane][j];
                    pw_t += s;
                    pw_p += s * s;
                }
                if (wf <= 2 * PT) { // the window's last tile: the gate of this block
                    const double dc_corr = len > 0 ? (pw_t * pw_t) / (double)len : 0.0;
                    double energy = pw_p - dc_corr;
                    energy = energy < 0.0 ? 0.0 : energy;
                    const float pwr = (float)(energy / (double)(len > 0 ? len : 1));
                    gate_l[cur.blk & 3][lane] = (pwr < a.squelch_level) ? 0 : 1;
                }
            } else if (cur.pass == 1) {
                const long g0 = cur.blk * block_len + (long)cur.tile * TS;
                const int tn = (bl - cur.tile * TS) < TS ? (bl - cur.tile * TS) : TS;
                if (cur.tile == 0) { // one envelope step per block
                    st.gate_open = gate_of(cur.blk, lane) ? 1 : 0;
                    const float target = st.gate_open ? 1.0f : 0.0f;
                    const float alpha = st.gate_open ? a.env_attack : a.env_release;
                    float env = st.squelch_env + alpha * (target - st.squelch_env);
                    env = env < 0.0f ? 0.0f : (env > 1.0f ? 1.0f : env);
                    st.squelch_env = env;
                }
                const int cnt = (int)(dec_upto(g0 + tn) - dec_upto(g0));
                const float env = st.squelch_env;
                int m = 0;
                for (int k = 0; k < cnt; k++) {
                    float v = tile[buf][lane][k];
                    if (a.deemph_on) {
                        const float d = v - st.deemph_avg;
                        st.deemph_avg += d * a.deemph_a;
                        v = st.deemph_avg;
                    }
                    if (a.lpf_on) {
                        const float d = v - st.audio_lpf_state;
                        st.audio_lpf_state += d * a.lpf_alpha;
                        v = st.audio_lpf_state;
                    }
                    if (a.dc_on) {
                        st.dc_avg += (v - st.dc_avg) * a.dc_scale;
                        v = v - st.dc_avg;
                    }
                    if (a.lpr_on) {
                        st.now_lpr += v;
                        lpr_index += a.lpr_slow;
                        if (lpr_index < a.lpr_fast) {
                            continue;
                        }
                        v = st.now_lpr * a.lpr_recip;
                        lpr_index -= a.lpr_fast;
                        st.now_lpr = 0.0f;
                    }
                    tile[buf][lane][64 + m] = v * env;
                    m++;
                }
            }
        }
        __syncthreads();
        prev = cur;
        have_prev_step = true;
        cur = nxt;
        more = has_next;
        buf ^= 1;
    }
    if (stager && have_prev_step) {
        flush(prev, buf ^ 1);
        if (M > 1) {
            for (int r = 0; r < RPW; r++) {
                const int c = row0 + r;
                if (lane < 16 && ch0 + c < a.n_channels) {
                    a.ring[(size_t)(ch0 + c) * 16 + lane] = hist[hp][c][lane];
                }
            }
        }
    }
    if (live && n > 0) {
        const f2 last = st.gate_open ? in[(size_t)ch * a.stride + (size_t)(n - 1)] : f2{0.0f, 0.0f};
        st.pre_r = last.x;
        st.pre_j = last.y;
        st.history_valid = 1;
        a.state[ch] = st;
    }
}
} // namespace

extern "C" hipError_t
ddn_dev_fm_audio(const DdnFmAudioArgs* args, hipStream_t st) {
    if (args->n_channels <= 0 || args->n <= 0) {
        return hipSuccess;
    }
    const size_t shm = sizeof(float) * 2 * 64 * (ROW + HW) + sizeof(int) * 4 * 64;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fm_audio), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e != hipSuccess) {
        return e;
    }
    hipLaunchKernelGGL(k_fm_audio, dim3((unsigned)((args->n_channels + 63) / 64)), dim3(64 * (1 + NSTAGE)), shm, st, *args);
    return hipGetLastError();
}
