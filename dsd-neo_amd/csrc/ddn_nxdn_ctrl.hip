// ddn_nxdn_ctrl.hip - NXDN frames that carry no SACCH / FACCH1 pair, and the SACCH superframe (include/ddn_fsk4.h, "NXDN control and
// data channels"): the outbound CAC of a control channel (LICH 0x01 / 0x05), FACCH2 (0x28, 0x29, 0x49) and UDCH (0x2E, 0x2F, 0x4E,
// 0x4F), and the running state nxdn_handle_sacch() keeps from frame to frame.
//
// reference: src/protocol/nxdn/nxdn_frame.c:117-160 (which LICH carries what), :237-263 (a LICH off the table resets the segment
// store), :311-346 (bit windows), :488-494 (non-superframe LICHs); nxdn_deperm.c:112-119,164-182 (de-permutation, 12-in-14
// de-puncture), :184-205 (soft decode, hard retry), :245-340 (SACCH), :496-530 (FACCH2 / UDCH), :610-634 (CAC), :1263-1275 (crc16cac),
// :1299-1372; nxdn_dcr_utils.c:44-106 (crc15, the sequence rule); nxdn_element.c:158-200 (NXDN_SACCH_Full_decode).
//
//   k_nxdn_ctrl_gather  one wavefront per sync slot: LICH -> kind; for a CAC / FACCH2 / UDCH frame record -> de-scrambled bit ->
//                       de-permuted index -> de-punctured index in closed form, straight into the rows the decoders take
//   (decoders)          k_k5_nxdn (soft, fresh metrics per word) and k_trellis_greedy under the two wanted masks the gather leaves
//   k_nxdn_ctrl_finish  CRC of the soft result, the reference's pick, verdict, RAN / SF, trellis_buf and m_data
//   k_nxdn_ctrl_walk    one lane per channel over its frames in air order: part_of_frame, the segment store, last RAN, cac_fail
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddn_crc_dev.h"
#include "ddn_device.h"

namespace {

// the PN9 sequence nxdn_descramble_with_seed(.., 182, 228) flips sign bits by (x^9 + x^4 + 1, nxdn_descramble.c:35-57): bit i of the
// table = dibit i, a compile-time constant
struct Pn9 {
    uint32_t w[6];
};
constexpr Pn9
make_pn9() {
    Pn9 p{};
    unsigned l = 228u;
    for (int i = 0; i < 182; i++) {
        p.w[i >> 5] |= (l & 1u) << (i & 31);
        const unsigned b = ((l >> 4) ^ l) & 1u;
        l = (l >> 1) | (b << 8);
    }
    return p;
}
__device__ const Pn9 k_pn9 = make_pn9();
static_assert((make_pn9().w[0] & 0xFFu) == 0xE4u, "the sequence starts 0 0 1 0 0 1 1 1");

__device__ __forceinline__ unsigned
pn9(int i) {
    return (k_pn9.w[i >> 5] >> (i & 31)) & 1u;
}

enum { KIND_NONE = 0, KIND_CAC = 1, KIND_FACCH2 = 2, KIND_UDCH = 3 };
constexpr int CAC_STEPS = 175, CAC_BITS = 171, F2_STEPS = 203, F2_BITS = 199;

// k_nxdn_lich_profiles (nxdn_frame.c:117-160) as sets over the 7-bit LICH: every row, the rows with sacch = 1
__device__ __forceinline__ bool
in_set(int lich, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3) {
    const uint32_t m = lich < 32 ? m0 : (lich < 64 ? m1 : (lich < 96 ? m2 : m3));
    return (m >> (lich & 31)) & 1u;
}
__device__ __forceinline__ bool
lich_in_profile(int lich) { // (the receive loop's gate, ddn_fsk4h_dev.h nxdn_lich_ok, holds the same set)
    return in_set(lich, 0x00000122u, 0x03FFC303u, 0x00FFC743u, 0x00EFC30Fu);
}
__device__ __forceinline__ bool
lich_has_sacch(int lich) { // 20 21 30..39 | 40 41 50..57
    return in_set(lich, 0u, 0x03FF0003u, 0x00FF0003u, 0u);
}
__device__ __forceinline__ int
lich_kind(int lich) {
    if (lich == 0x01 || lich == 0x05) {
        return KIND_CAC;
    }
    if (lich == 0x28 || lich == 0x29 || lich == 0x49) {
        return KIND_FACCH2;
    }
    if (lich == 0x2E || lich == 0x2F || lich == 0x4E || lich == 0x4F) {
        return KIND_UDCH;
    }
    return KIND_NONE;
}

// One wavefront per sync slot, four slots per workgroup.  A slot that holds no whole frame, a LICH whose parity fails or one that
// names another channel costs the eight LICH records and writes its kind (0) and its two wanted flags.
__global__ __launch_bounds__(256) void
k_nxdn_ctrl_gather(const uint8_t* __restrict__ rec, const int32_t* __restrict__ counts, size_t max_sym,
                   const int32_t* __restrict__ sync_pos, const int32_t* __restrict__ n_sync, int n_channels, int max_sync,
                   uint8_t* __restrict__ kind, uint8_t* __restrict__ sym_c, uint8_t* __restrict__ rel_c, uint8_t* __restrict__ hard_c,
                   uint8_t* __restrict__ sym_f, uint8_t* __restrict__ rel_f, uint8_t* __restrict__ hard_f,
                   uint8_t* __restrict__ want_c, uint8_t* __restrict__ want_f) {
    const int lane = threadIdx.x & 63;
    const size_t so = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (so >= (size_t)n_channels * (size_t)max_sync) {
        return;
    }
    const int ch = (int)(so / (size_t)max_sync), k = (int)(so % (size_t)max_sync);
    const bool have = k < n_sync[ch];
    const long pos = have ? sync_pos[so] : 0;
    const bool ok = have && pos >= 0 && (pos + 182 < (long)counts[ch]) && ((size_t)(pos + 182) < max_sym);
    const uint8_t* fr = rec + ((size_t)ch * max_sym + (size_t)(ok ? pos + 1 : 0)) * 10; // the frame's 182 records
    int kd = KIND_NONE;
    if (ok) {
        // nxdn_collect_lich / nxdn_prepare_lich_parity: the first eight dibits' high bits, first dibit in bit 7
        const unsigned hi = lane < 8 ? ((((unsigned)fr[lane * 10] >> 1) & 1u) ^ pn9(lane)) : 0u;
        const unsigned long long m = __ballot(hi != 0);
        int l = 0;
        for (int i = 0; i < 8; i++) {
            l |= (int)((m >> i) & 1ull) << (7 - i);
        }
        const int l7 = l >> 1;
        int par = ((l >> 7) + (l >> 6) + (l >> 5) + (l >> 4)) & 1;
        if (l7 == 0x08 || l7 == 0x4A || l7 == 0x48 || l7 == 0x46) {
            par = ((l >> 7) + (l >> 6) + (l >> 5) + (l >> 4) + (l >> 3) + (l >> 2) + (l >> 1)) & 1;
        }
        if ((l & 1) == par && lich_in_profile(l7)) {
            kd = lich_kind(l7);
        }
    }
    if (lane == 0) {
        kind[so] = (uint8_t)kd;
        want_c[so] = kd == KIND_CAC;
        want_f[so] = kd == KIND_FACCH2 || kd == KIND_UDCH;
    }
    if (kd == KIND_NONE) {
        return;
    }
    // bits 16 .. 16 + nb of the de-scrambled frame; PERM_12_N[i] = (i % N) * 12 + i / N (nxdn_const.h:41-70); of every twelve
    // de-permuted bits fourteen: {0 1 2 - 3 4 5 6 7 8 9 - 10 11} (nxdn_depuncture_12_group_rel)
    const int N = kd == KIND_CAC ? 25 : 29, nb = 12 * N;
    uint8_t* sym = kd == KIND_CAC ? sym_c + so * (size_t)(2 * CAC_STEPS) : sym_f + so * (size_t)(2 * F2_STEPS);
    uint8_t* rel = kd == KIND_CAC ? rel_c + so * (size_t)(2 * CAC_STEPS) : rel_f + so * (size_t)(2 * F2_STEPS);
    uint8_t* hard = kd == KIND_CAC ? hard_c + so * (size_t)(2 * CAC_STEPS) : hard_f + so * (size_t)(2 * F2_STEPS);
    for (int i = lane; i < nb; i += 64) {
        const int d = 8 + (i >> 1);
        const uint8_t* rr = fr + d * 10;
        const unsigned dib = ((unsigned)rr[0] & 3u) ^ (pn9(d) << 1);
        const unsigned b = (i & 1) ? (dib & 1u) : (dib >> 1);
        const int p = (i % N) * 12 + i / N;
        const int g = p / 12, m = p - g * 12;
        const int q = g * 14 + (m < 3 ? m : (m < 10 ? m + 1 : m + 2));
        sym[q] = (uint8_t)(b << 1);
        rel[q] = rr[1]; // one reliability per dibit, used for both of its bits
        hard[q] = (uint8_t)b;
    }
    for (int e = lane; e < 2 * N; e += 64) { // the erasures: bit 0, reliability 0
        const int q = (e >> 1) * 14 + ((e & 1) ? 11 : 3);
        sym[q] = 0;
        rel[q] = 0;
        hard[q] = 0;
    }
}

// One lane per slot.  soft: the K = 5 decoder's packed rows (stride 26), hard: the greedy decoder's rows of one bit per byte
// (stride 208).  nxdn_deperm_cac_soft / nxdn_deperm_facch2_udch_soft behind the decodes: the soft result where its CRC holds, else
// the hard one whatever its CRC says.
__global__ void
k_nxdn_ctrl_finish(const uint8_t* __restrict__ kind, const uint8_t* __restrict__ soft_c, const uint8_t* __restrict__ soft_f,
                   const uint8_t* __restrict__ hard_c, const uint8_t* __restrict__ hard_f, size_t n, uint8_t* __restrict__ bits208,
                   uint8_t* __restrict__ bytes26, uint8_t* __restrict__ crc_ok, uint8_t* __restrict__ fallback,
                   uint8_t* __restrict__ ran, uint8_t* __restrict__ sf) {
    const size_t so = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (so >= n) {
        return;
    }
    const int kd = kind[so];
    if (kd == KIND_NONE) { // its rows stay as they were
        return;
    }
    const bool cac = kd == KIND_CAC;
    const int nbits = cac ? CAC_BITS : F2_BITS, nbytes = cac ? 22 : 26;
    const uint8_t* sb = (cac ? soft_c : soft_f) + so * 26;
    const uint8_t* hb = (cac ? hard_c : hard_f) + so * 208;
    // crc16cac over the 171 bits must be 0: the register from 0xC3EE over the first 155 equals the 16 behind them; crc15 over bits
    // 0..183 against bits 184..198
    auto good = [&](auto get) {
        if (cac) {
            uint32_t f = 0;
            for (int i = 155; i < 171; i++) {
                f = (f << 1) | get(i);
            }
            return ddn_crc::of_bits(ddn_crc::NXDN_CRC16CAC, 155, get) == f;
        }
        uint32_t f = 0;
        for (int i = 184; i < 199; i++) {
            f = (f << 1) | get(i);
        }
        return ddn_crc::of_bits(ddn_crc::NXDN_CRC15, 184, get) == f;
    };
    auto soft_bit = [&](int i) { return (uint32_t)((sb[i >> 3] >> (7 - (i & 7))) & 1u); };
    auto hard_bit = [&](int i) { return (uint32_t)(hb[i] & 1u); };
    const bool soft_ok = good(soft_bit);
    const bool ok = soft_ok || good(hard_bit);
    auto bit = [&](int i) { return i < nbits ? (soft_ok ? soft_bit(i) : hard_bit(i)) : 0u; };
    if (bits208) {
        for (int i = 0; i < 208; i++) {
            bits208[so * 208 + i] = (uint8_t)bit(i);
        }
    }
    if (bytes26) {
        for (int j = 0; j < 26; j++) {
            uint32_t v = 0;
            for (int i = 0; i < 8; i++) {
                v = (v << 1) | bit(8 * j + i);
            }
            bytes26[so * 26 + j] = (uint8_t)(j < nbytes ? v : 0u);
        }
    }
    if (crc_ok) {
        crc_ok[so] = ok;
    }
    if (fallback) {
        fallback[so] = !soft_ok;
    }
    if (ran) {
        ran[so] = (uint8_t)((bit(2) << 5) | (bit(3) << 4) | (bit(4) << 3) | (bit(5) << 2) | (bit(6) << 1) | bit(7));
    }
    if (sf) {
        sf[so] = (uint8_t)((bit(0) << 1) | bit(1));
    }
}

// what the reference keeps in dsd_state between two NXDN frames (and in nxdn_deperm.c's cac_fail)
struct CtrlState {
    int32_t part_of_frame, last_ran, cac_fail; // last_ran: -1 = none
    uint8_t segcrc[4];
    uint8_t segment[4][18];
};

__device__ __forceinline__ void
reset_segments(CtrlState& s) { // nxdn_reset_sacch_segments: both start at 1
    for (int p = 0; p < 4; p++) {
        s.segcrc[p] = 1;
        for (int i = 0; i < 18; i++) {
            s.segment[p][i] = 1;
        }
    }
}

__global__ void
k_nxdn_ctrl_state_init(CtrlState* __restrict__ st, int n_channels) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_channels) {
        return;
    }
    CtrlState s;
    s.part_of_frame = 0;
    s.last_ran = -1;
    s.cac_fail = 0;
    reset_segments(s);
    st[ch] = s;
}

// One lane per channel, its slots in air order.  Per frame, in the reference's order: the profile-miss reset (a parity failure
// leaves the store alone), the SACCH mode of the LICH, for a SACCH frame the pick between the soft decode and the greedy retry and
// nxdn_handle_sacch(), for a CAC / FACCH2 / UDCH frame what its handler does to part_of_frame, last RAN and cac_fail.
__global__ void
k_nxdn_ctrl_walk(const int32_t* __restrict__ n_sync, int n_channels, int max_sync, const uint8_t* __restrict__ lich,
                 const uint8_t* __restrict__ valid, const uint8_t* __restrict__ sacch, const uint8_t* __restrict__ sacch_ok,
                 const uint8_t* __restrict__ sacch_hard, const uint8_t* __restrict__ sacch_hard_ok, const uint8_t* __restrict__ kind,
                 const uint8_t* __restrict__ crc_ok, const uint8_t* __restrict__ ran, const uint8_t* __restrict__ sf,
                 CtrlState* __restrict__ state, uint8_t* __restrict__ sacch_status, uint8_t* __restrict__ pf, uint8_t* __restrict__ seq_ok,
                 uint8_t* __restrict__ msg72, uint8_t* __restrict__ msg_status, int32_t* __restrict__ last_ran,
                 int32_t* __restrict__ cac_fail) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_channels) {
        return;
    }
    CtrlState s = state[ch];
    const int ns = n_sync[ch] < max_sync ? n_sync[ch] : max_sync;
    for (int k = 0; k < ns; k++) {
        const size_t so = (size_t)ch * max_sync + k;
        int status = 0, seq = 0, mst = 0, fails = s.cac_fail;
        const int l = lich[so], l7 = l & 0x7F;
        if (valid[so] && (l & 0x80)) {
            if (!lich_in_profile(l7)) {
                reset_segments(s);
            } else if (lich_has_sacch(l7)) {
                uint8_t t[32];
                const bool soft = sacch_ok[so] != 0;
                for (int i = 0; i < 32; i++) {
                    t[i] = soft ? (uint8_t)((sacch[so * 4 + (i >> 3)] >> (7 - (i & 7))) & 1u) : (uint8_t)(sacch_hard[so * 32 + i] & 1u);
                }
                const bool good = soft || sacch_hard_ok[so] != 0;
                const int r = (t[2] << 5) | (t[3] << 4) | (t[4] << 3) | (t[5] << 2) | (t[6] << 1) | t[7];
                if (!good) {
                    reset_segments(s);
                }
                if (l7 == 0x20 || l7 == 0x21 || l7 == 0x61 || l7 == 0x40 || l7 == 0x41) { // nxdn_handle_sacch_non_superframe
                    if (good) {
                        s.last_ran = r;
                    }
                    s.part_of_frame = good ? 3 : 0;
                    status = good ? 3 : 4;
                    seq = good;
                    mst = good;
                    if (msg72) {
                        for (int i = 0; i < 72; i++) {
                            msg72[so * 72 + i] = i < 24 ? t[8 + i] : 0;
                        }
                    }
                    reset_segments(s);
                } else { // nxdn_handle_sacch_superframe
                    const int f = (t[0] << 1) | t[1];
                    const int part = f == 2 ? 1 : (f == 1 ? 2 : (f == 0 ? 3 : 0));
                    seq = good && (part == 0 || part == ((s.part_of_frame + 1) & 3));
                    if (!seq) {
                        reset_segments(s);
                    }
                    s.part_of_frame = part;
                    if (good) {
                        s.last_ran = r;
                    }
                    s.segcrc[part] = good ? 0 : 1;
                    for (int i = 0; i < 18; i++) {
                        s.segment[part][i] = t[8 + i];
                    }
                    status = good ? 1 : 2;
                    if (part == 3) { // NXDN_SACCH_Full_decode: delivered when all four CRCs were good, the store reset either way
                        mst = (s.segcrc[0] | s.segcrc[1] | s.segcrc[2] | s.segcrc[3]) ? 2 : 1;
                        if (msg72) {
                            for (int i = 0; i < 72; i++) {
                                msg72[so * 72 + i] = s.segment[i / 18][i % 18];
                            }
                        }
                        reset_segments(s);
                    }
                }
            } else if (kind[so] == KIND_CAC) { // nxdn_handle_cac, nxdn_update_cac_fail_state
                if (crc_ok[so]) {
                    s.last_ran = ran[so];
                    s.cac_fail = fails = 0;
                } else {
                    fails = s.cac_fail + 1;
                    // above ten the reference resets its symbolizer and the counter; here the counter alone (the frame reports 11)
                    s.cac_fail = fails > 10 ? 0 : fails;
                }
            } else if (kind[so] != KIND_NONE) { // nxdn_handle_facch2_udch
                if (crc_ok[so]) {
                    s.last_ran = ran[so];
                    s.part_of_frame = 3 - sf[so];
                } else {
                    s.part_of_frame = 0;
                }
            }
        }
        if (sacch_status) {
            sacch_status[so] = (uint8_t)status;
        }
        if (pf) {
            pf[so] = (uint8_t)s.part_of_frame;
        }
        if (seq_ok) {
            seq_ok[so] = (uint8_t)seq;
        }
        if (msg_status) {
            msg_status[so] = (uint8_t)mst;
        }
        if (last_ran) {
            last_ran[so] = s.last_ran;
        }
        if (cac_fail) {
            cac_fail[so] = fails;
        }
    }
    state[ch] = s;
}

} // namespace

extern "C" size_t
ddn_dev_nxdn_ctrl_state_bytes(void) {
    return sizeof(CtrlState);
}

extern "C" hipError_t
ddn_dev_nxdn_ctrl_state_init(void* state, int n_channels, hipStream_t st) {
    hipLaunchKernelGGL(k_nxdn_ctrl_state_init, dim3((unsigned)((n_channels + 63) / 64)), dim3(64), 0, st, (CtrlState*)state, n_channels);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_nxdn_ctrl_gather(const uint8_t* rec, const int32_t* counts, size_t max_sym, const int32_t* sync_pos, const int32_t* n_sync,
                         int n_channels, int max_sync, uint8_t* kind, uint8_t* sym_c, uint8_t* rel_c, uint8_t* hard_c, uint8_t* sym_f,
                         uint8_t* rel_f, uint8_t* hard_f, uint8_t* want_c, uint8_t* want_f, hipStream_t st) {
    const size_t S = (size_t)n_channels * (size_t)max_sync;
    hipLaunchKernelGGL(k_nxdn_ctrl_gather, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, rec, counts, max_sym, sync_pos, n_sync, n_channels,
                       max_sync, kind, sym_c, rel_c, hard_c, sym_f, rel_f, hard_f, want_c, want_f);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_nxdn_ctrl_finish(const uint8_t* kind, const uint8_t* soft_c, const uint8_t* soft_f, const uint8_t* hard_c, const uint8_t* hard_f,
                         size_t n, uint8_t* bits208, uint8_t* bytes26, uint8_t* crc_ok, uint8_t* fallback, uint8_t* ran, uint8_t* sf,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_nxdn_ctrl_finish, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, kind, soft_c, soft_f, hard_c, hard_f, n, bits208,
                       bytes26, crc_ok, fallback, ran, sf);
    return hipGetLastError();
}

extern "C" hipError_t
ddn_dev_nxdn_ctrl_walk(const int32_t* n_sync, int n_channels, int max_sync, const uint8_t* lich, const uint8_t* valid, const uint8_t* sacch,
                       const uint8_t* sacch_ok, const uint8_t* sacch_hard, const uint8_t* sacch_hard_ok, const uint8_t* kind,
                       const uint8_t* crc_ok, const uint8_t* ran, const uint8_t* sf, void* state, uint8_t* sacch_status, uint8_t* pf,
                       uint8_t* seq_ok, uint8_t* msg72, uint8_t* msg_status, int32_t* last_ran, int32_t* cac_fail, hipStream_t st) {
    hipLaunchKernelGGL(k_nxdn_ctrl_walk, dim3((unsigned)((n_channels + 63) / 64)), dim3(64), 0, st, n_sync, n_channels, max_sync, lich, valid,
                       sacch, sacch_ok, sacch_hard, sacch_hard_ok, kind, crc_ok, ran, sf, (CtrlState*)state, sacch_status, pf, seq_ok, msg72,
                       msg_status, last_ran, cac_fail);
    return hipGetLastError();
}
