// ddn_api_rx4.cpp - C-ABI of the batched fsk4 receive loop (include/ddn_fsk4.h, kernels ddn_rx4.hip).  What a protocol is stands in
// its row of ddn_fsk4::kRow (ddn_fsk4_proto.h): create() checks a configuration against the row and builds the profile a batch runs
// (the batch's choices and the row's sync words) from {protocol, rf_mod, inverted}; per-channel decoder words live on the device
// inside the batch object and persist across calls.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ddn_api_util.h"
#include "ddn_device.h"
#include "ddn_fsk4.h"
#include "ddn_fsk4_proto.h"

using namespace ddn_fsk4;
static_assert(MAX_ROW_PAT <= DDN_FSK4_MAX_PAT, "a row's patterns fit the profile");

// pattern k of a protocol that accepts ddn_fsk4_rx_config::inverted, as it is hunted with inverted set
static Pat
inverted_pat(int protocol, int k, Pat p) {
    if (protocol == DDN_FSK4_DPMR) { // -xd: the inverted FS2 word
        p.complement = true;
        p.type = T_DPMR_FS2_INV;
    } else if (k == DDN_FSK4_DMR_RC_PAT) { // -xr claims the RC word's complement (sync_patterns.h:74-75)
        p.complement = true;
    } else { // frame_sync_try_dmr_*: the data word marks an inverted voice burst and vice versa
        p.cls ^= 1;
        if (p.type == T_BS_DATA) {
            p.type = T_BS_VOICE_NEG;
            p.neg = 1;
        } else if (p.type == T_BS_VOICE) {
            p.type = T_BS_DATA_NEG;
            p.neg = 1;
        } else {
            p.type = (p.type == T_MS_DATA) ? T_MS_VOICE : T_MS_DATA; // MS types carry no digitize() polarity
        }
    }
    return p;
}

struct ddn_fsk4_rx {
    ddn_fsk4_rx_config cfg;
    DdnFsk4Config dc;
    DdnFsk4State* d_state;
    float *d_lbuf, *d_shist, *d_fhist, *d_fstale, *d_filt, *d_taps;
    DdnFsk4Config* d_cfg;
    uint8_t *d_phist, *d_rhist;
    int32_t* d_lock;
    size_t filt_cap;
    int channels_per_wave;
    int dbg_flags; // ddn_fsk4_rx_set_debug_flags
    // handler mode (ddn_fsk4_rx_set_handlers): the handlers' words [B][32] i32, the burst's dibits [B][144], event buffers
    int32_t* d_hwords;
    uint8_t* d_hpay;
    int32_t *d_events, *d_n_events;
    size_t max_events;
    int32_t *d_ev_own, *d_nev_own; // event buffers of the host convenience calls (ddn_fsk4_rx_events_host_*)
    const Row* row;                // the protocol
    bool timing;
    hipEvent_t ev[3];
    DdnPool pool;
};

static void
rx4_free(ddn_fsk4_rx* b) {
    b->pool.release();
    for (int i = 0; i < 3; i++) {
        if (b->ev[i]) {
            (void)hipEventDestroy(b->ev[i]);
        }
    }
}

static int
rx4_fill(ddn_fsk4_rx* b) {
    const size_t B = (size_t)b->cfg.n_channels;
    DdnFsk4State s0;
    memset(&s0, 0, sizeof(s0));
    s0.jitter = -1;
    // symbol_reset_rtl_fsk_timing_if_needed() + symbol_reset_rtl_fsk_discriminator_slicer() (dsd_symbol.c:1306-1341)
    s0.center = 0.0f;
    s0.min = -30000.0f;
    s0.max = 30000.0f;
    s0.lmid = -20000.0f;
    s0.umid = 20000.0f;
    s0.minref = -24000.0f;
    s0.maxref = 24000.0f;
    s0.lmin = s0.min;
    s0.lmax = s0.max;
    std::vector<DdnFsk4State> st(B, s0);
    HIP_TRY(hipMemcpy(b->d_state, st.data(), sizeof(DdnFsk4State) * B, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b->d_lbuf, 0, sizeof(float) * 24 * B));
    HIP_TRY(hipMemset(b->d_shist, 0, sizeof(float) * DDN_FSK4_HIST * B));
    HIP_TRY(hipMemset(b->d_phist, 0, DDN_FSK4_HIST * B));
    HIP_TRY(hipMemset(b->d_rhist, 0, DDN_FSK4_HIST * B));
    HIP_TRY(hipMemset(b->d_fhist, 0, sizeof(float) * (DDN_FSK4_MAX_TAPS - 1) * B));
    HIP_TRY(hipMemset(b->d_fstale, 0, sizeof(float) * (DDN_FSK4_MAX_TAPS - 1) * B));
    {   // dmr_confidence_reset() + state->dmr_color_code = 16 (dsd_init.c:1099): field order of ddn_fsk4h_dev.h
        std::vector<int32_t> hw(32 * B, 0);
        for (size_t c = 0; c < B; c++) {
            hw[32 * c + 1] = 16;  // F_CONF_CC
            hw[32 * c + 2] = 16;  // F_CAND_CC
            hw[32 * c + 11] = 16; // F_COLOR
        }
        HIP_TRY(hipMemcpy(b->d_hwords, hw.data(), sizeof(int32_t) * 32 * B, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(b->d_hpay, 0, 144 * B));
    }
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_create(const ddn_fsk4_rx_config* cfg, ddn_fsk4_rx** out) {
    if (!cfg || !out) {
        return DDN_EINVAL;
    }
    *out = nullptr;
    if (cfg->n_channels <= 0 || cfg->out_rate_hz <= 0 || !known(cfg->protocol) || (cfg->rf_mod != 0 && cfg->rf_mod != 2)
        || (cfg->inverted && !kRow[cfg->protocol].inverted_ok)) {
        ddn_set_error("ddn_fsk4_rx_create: bad configuration (protocol DMR | NXDN48 | NXDN96 | M17 | YSF | DPMR | DSTAR | EDACS, "
                      "rf_mod 0 | 2, inverted only for DMR and DPMR)");
        return DDN_EINVAL;
    }
    const Row& r = kRow[cfg->protocol];
    const int sps = cfg->out_rate_hz / r.sym_rate;
    if (sps < r.sps_min || sps > r.sps_max || (r.sps_whole && cfg->out_rate_hz % r.sym_rate != 0)) {
        ddn_set_error(r.sps_whole ? "ddn_fsk4_rx_create: EDACS needs out_rate_hz = 9600 x 5..10 (48 ksps: 5 samples per symbol)"
                                  : "ddn_fsk4_rx_create: out_rate_hz / symbol rate must be within 8..21 (48 ksps: DMR 10, NXDN48 20)");
        return DDN_ERANGE;
    }
    DDN_TRY(ddn_have_device());
    ddn_fsk4_rx* b = new (std::nothrow) ddn_fsk4_rx();
    if (!b) {
        return DDN_ENOMEM;
    }
    memset(b, 0, sizeof(*b));
    b->cfg = *cfg;
    b->row = &r;
    DdnFsk4Config& d = b->dc;
    d.out_rate = cfg->out_rate_hz;
    d.rf_mod = cfg->rf_mod;
    d.use_filter = (cfg->use_matched_filter && r.taps != TAPS_NONE) ? 1 : 0;
    for (int k = 0; k < r.n_pat(); k++) {
        const Pat p = cfg->inverted ? inverted_pat(cfg->protocol, k, r.pat[k]) : r.pat[k];
        const uint64_t bits = word_bits(p.word, p.complement);
        d.pat_bits[k] = (uint32_t)(bits & 0xFFFFFFu);
        d.pat_hi[k] = (uint32_t)(bits >> 24);
        d.pat_type[k] = p.type;
        d.pat_class[k] = p.cls;
        d.pat_neg[k] = p.neg;
    }
    bool all_zero = true;
    for (int k = 0; k < 4; k++) {
        all_zero = all_zero && cfg->lock_symbols[k] == 0;
    }
    for (int k = 0; k < 4; k++) {
        b->cfg.lock_symbols[k] = all_zero ? r.lock_symbols[k] : cfg->lock_symbols[k];
    }
    const size_t B = (size_t)cfg->n_channels;
    // fewer channels per wavefront = fewer unsynchronised recurrences sharing one instruction stream, and a trip is only a
    // lean trip when every lane of the wave is inside a frame (measured at 4096 DMR channels: 11.8 ms with 4 lanes per wave,
    // 13.6 with 8, 16.7 with 16); two-wave workgroups, so 4096 channels at 4 per wave are eight wavefronts per CU
    // (round 3, with the bulk hunting pass: at 1365 channels 9.5 / 7.6 / 6.2 ms DMR and 6.5 / 4.0 / 2.6 ms NXDN48 with 4 / 2 / 1
    // lanes per wave - as long as all the workgroups are resident at once: 2048 one-channel workgroups run in two rounds)
    b->channels_per_wave = 32;
    for (int cpw = 1; cpw <= 32; cpw *= 2) {
        if ((B + cpw - 1) / cpw <= 1536) {
            b->channels_per_wave = cpw;
            break;
        }
    }
    if (const char* e = DDN_EXP_ENV("DDN_RX4_CPW")) { // (experiments; the same values ddn_fsk4_rx_set_channels_per_wave accepts)
        const int v = atoi(e);
        if (v >= 1 && v <= 32 && (v & (v - 1)) == 0) {
            b->channels_per_wave = v;
        }
    }
    std::vector<int32_t> lock(B * 4);
    for (size_t c = 0; c < B; c++) {
        for (int k = 0; k < 4; k++) {
            lock[c * 4 + k] = b->cfg.lock_symbols[k];
        }
    }
    float taps[DDN_FSK4_MAX_TAPS] = {0};
    if (const unsigned int* tap_bits = taps_bits(r.taps)) {
        memcpy(taps, tap_bits, sizeof(float) * (size_t)taps_len(r.taps));
    }
    DdnPool& p = b->pool;
    if (!p.alloc(&b->d_state, B) || !p.alloc(&b->d_lbuf, 24 * B) || !p.alloc(&b->d_shist, DDN_FSK4_HIST * B) || !p.alloc(&b->d_phist, DDN_FSK4_HIST * B)
        || !p.alloc(&b->d_rhist, DDN_FSK4_HIST * B) || !p.alloc(&b->d_fhist, (DDN_FSK4_MAX_TAPS - 1) * B)
        || !p.alloc(&b->d_fstale, (DDN_FSK4_MAX_TAPS - 1) * B) || !p.alloc(&b->d_taps, DDN_FSK4_MAX_TAPS) || !p.alloc(&b->d_cfg, 1)
        || hipMemcpy(b->d_cfg, &b->dc, sizeof(DdnFsk4Config), hipMemcpyHostToDevice) != hipSuccess || !p.alloc(&b->d_lock, 4 * B)
        || !p.alloc(&b->d_hwords, 32 * B) || !p.alloc(&b->d_hpay, 144 * B)
        || hipMemcpy(b->d_taps, taps, sizeof(taps), hipMemcpyHostToDevice) != hipSuccess
        || hipMemcpy(b->d_lock, lock.data(), sizeof(int32_t) * 4 * B, hipMemcpyHostToDevice) != hipSuccess) {
        ddn_set_error("ddn_fsk4_rx_create: device allocation failed");
        rx4_free(b);
        delete b;
        return DDN_ENOMEM;
    }
    const int rc = rx4_fill(b);
    if (rc != DDN_OK) {
        rx4_free(b);
        delete b;
        return rc;
    }
    *out = b;
    return DDN_OK;
}

extern "C" void
ddn_fsk4_rx_destroy(ddn_fsk4_rx* b) {
    if (b) {
        rx4_free(b);
        delete b;
    }
}

extern "C" int
ddn_fsk4_rx_set_handlers(ddn_fsk4_rx* b, int enable) {
    if (!b) {
        return DDN_EINVAL;
    }
    if (enable && b->cfg.inverted) {
        ddn_set_error("ddn_fsk4_rx_set_handlers: the handlers are the reference's plain -fs ones (inverted = 0)");
        return DDN_EINVAL;
    }
    if (enable && !b->row->handlers) {
        ddn_set_error("ddn_fsk4_rx_set_handlers: %s reads fixed counts behind a sync (no handler family)", b->row->name);
        return DDN_EINVAL;
    }
    b->dc.handlers = enable ? 1 : 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(b->d_cfg, &b->dc, sizeof(DdnFsk4Config), hipMemcpyHostToDevice));
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_set_events(ddn_fsk4_rx* b, int32_t* d_events, int32_t* d_n_events, size_t max_events) {
    if (!b || ((d_events == nullptr) != (d_n_events == nullptr)) || (d_events && max_events == 0) || max_events > 0x7FFFFFFF) {
        return DDN_EINVAL;
    }
    b->d_events = d_events;
    b->d_n_events = d_n_events;
    b->max_events = d_events ? max_events : 0;
    b->dc.max_events = (int)b->max_events;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(b->d_cfg, &b->dc, sizeof(DdnFsk4Config), hipMemcpyHostToDevice));
    return DDN_OK;
}

// host convenience: event buffers owned by the batch object, read back after a run
extern "C" int
ddn_fsk4_rx_events_host_arm(ddn_fsk4_rx* b, size_t max_events) {
    if (!b || max_events == 0 || max_events > 0x7FFFFFFF) {
        return DDN_EINVAL;
    }
    const size_t B = (size_t)b->cfg.n_channels;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(b->pool.realloc_bytes(&b->d_ev_own, B * max_events * 16));
    HIP_TRY(b->pool.realloc_bytes(&b->d_nev_own, B * 4));
    HIP_TRY(hipMemset(b->d_ev_own, 0, B * max_events * 16));
    HIP_TRY(hipMemset(b->d_nev_own, 0, B * 4));
    return ddn_fsk4_rx_set_events(b, b->d_ev_own, b->d_nev_own, max_events);
}

extern "C" int
ddn_fsk4_rx_events_host_read(ddn_fsk4_rx* b, int32_t* events, int32_t* n_events) {
    if (!b || !events || !n_events || !b->d_ev_own || b->d_events != b->d_ev_own) {
        return DDN_EINVAL;
    }
    const size_t B = (size_t)b->cfg.n_channels;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(events, b->d_ev_own, B * b->max_events * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_events, b->d_nev_own, B * 4, hipMemcpyDeviceToHost));
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_reset(ddn_fsk4_rx* b) {
    if (!b) {
        return DDN_EINVAL;
    }
    HIP_TRY(hipDeviceSynchronize());
    return rx4_fill(b);
}

extern "C" size_t
ddn_fsk4_rx_max_symbols(const ddn_fsk4_rx* b, size_t n) {
    if (!b) {
        return 0;
    }
    int whole = b->dc.out_rate / b->row->sym_rate;
    whole = whole < 2 ? 2 : (whole > 64 ? 64 : whole);
    return n / (size_t)(whole - 1) + 2;
}

extern "C" size_t
ddn_fsk4_rx_max_syncs(const ddn_fsk4_rx* b, size_t n) {
    if (!b) {
        return 0;
    }
    // two accepted syncs are at least one sync window apart (the hunt restarts with an empty window)
    return ddn_fsk4_rx_max_symbols(b, n) / (size_t)b->row->win_len() + 2;
}

extern "C" int
ddn_fsk4_rx_set_lock_symbols(ddn_fsk4_rx* b, const int32_t* lock4) {
    if (!b || !lock4) {
        return DDN_EINVAL;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(b->d_lock, lock4, sizeof(int32_t) * 4 * (size_t)b->cfg.n_channels, hipMemcpyHostToDevice));
    return DDN_OK;
}

static int
check_fsk4_rx_run(const char* who, const ddn_fsk4_rx* b, const float* disc, const uint8_t* records10, const uint8_t* flags, const uint8_t* payload2,
                  const int32_t* counts, const int32_t* sync_pos, const uint8_t* sync_pat, const uint8_t* pre, const uint8_t* pre_rel,
                  const int32_t* n_sync) {
    return (b && disc && records10 && flags && payload2 && counts && sync_pos && sync_pat && pre && pre_rel && n_sync) ? DDN_OK
                                                                                                                        : ddn_bad_argument(who);
}

extern "C" int
ddn_fsk4_rx_run(ddn_fsk4_rx* b, const float* d_disc, size_t n, uint8_t* d_records10, uint8_t* d_flags, uint8_t* d_payload2,
                int32_t* d_counts, size_t max_symbols, int32_t* d_sync_pos, uint8_t* d_sync_pat, uint8_t* d_pre,
                uint8_t* d_pre_rel, int32_t* d_n_sync, size_t max_syncs, void* hip_stream) {
    DDN_TRY(check_fsk4_rx_run(__func__, b, d_disc, d_records10, d_flags, d_payload2, d_counts, d_sync_pos, d_sync_pat, d_pre, d_pre_rel, d_n_sync));
    hipStream_t st = (hipStream_t)hip_stream;
    const int B = b->cfg.n_channels;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * (size_t)B, st));
        HIP_TRY(hipMemsetAsync(d_n_sync, 0, sizeof(int32_t) * (size_t)B, st));
        return DDN_OK;
    }
    if (max_symbols < ddn_fsk4_rx_max_symbols(b, n) || max_syncs < ddn_fsk4_rx_max_syncs(b, n)) {
        ddn_set_error("ddn_fsk4_rx_run: max_symbols %zu / max_syncs %zu below ddn_fsk4_rx_max_symbols / _max_syncs (%zu / %zu)",
                      max_symbols, max_syncs, ddn_fsk4_rx_max_symbols(b, n), ddn_fsk4_rx_max_syncs(b, n));
        return DDN_ERANGE;
    }
    if (b->timing) {
        HIP_TRY(hipEventRecord(b->ev[0], st));
    }
    if (b->dc.use_filter) {
        if (b->filt_cap < n) {
            HIP_TRY(hipStreamSynchronize(st));
            b->filt_cap = 0;
            HIP_TRY(b->pool.realloc_bytes(&b->d_filt, sizeof(float) * (size_t)B * n));
            b->filt_cap = n;
        }
        HIP_TRY(ddn_dev_fsk4_matched_filter(b->row->taps, d_disc, (long)n, n, B, b->d_fhist, b->d_filt, st));
    }
    if (b->timing) {
        HIP_TRY(hipEventRecord(b->ev[1], st));
    }
    {
        int want = b->dbg_flags;
        if (const char* e = DDN_EXP_ENV("DDN_RX4_DBG")) {
            want = atoi(e);
        }
        if (b->dc.dbg != want) {
            b->dc.dbg = want;
            HIP_TRY(hipMemcpy(b->d_cfg, &b->dc, sizeof(DdnFsk4Config), hipMemcpyHostToDevice));
        }
    }
    DdnFsk4RxArgs a = {};
    a.raw = d_disc;
    a.filt = b->d_filt;
    a.prev_tail = b->d_fhist;
    a.fstale = b->d_fstale;
    a.taps = b->d_taps;
    a.n = (long)n;
    a.stride = n;
    a.n_channels = B;
    a.cfg = b->d_cfg;
    a.state = b->d_state;
    a.lbuf_store = b->d_lbuf;
    a.shist_store = b->d_shist;
    a.phist_store = b->d_phist;
    a.rhist_store = b->d_rhist;
    a.rec = d_records10;
    a.flags = d_flags;
    a.pay = d_payload2;
    a.counts = d_counts;
    a.max_sym = max_symbols;
    a.lock4 = b->d_lock;
    a.sync_pos = d_sync_pos;
    a.sync_pat = d_sync_pat;
    a.pre = d_pre;
    a.pre_rel = d_pre_rel;
    a.n_sync = d_n_sync;
    a.max_sync = (int)max_syncs;
    a.channels_per_wave = b->channels_per_wave;
    a.samples_per_symbol = (b->dc.out_rate + b->row->sym_rate - 1) / b->row->sym_rate;
    a.protocol = b->cfg.protocol;
    a.handlers = b->dc.handlers;
    a.hwords = b->d_hwords;
    a.hpay = b->d_hpay;
    a.events = b->d_events;
    a.n_events = b->d_n_events;
    HIP_TRY(ddn_dev_fsk4_rx(&a, st));
    if (b->timing) {
        HIP_TRY(hipEventRecord(b->ev[2], st));
    }
    HIP_TRY(ddn_dev_fsk4_filter_hist_update(b->row->taps, d_disc, (long)n, n, B, b->d_fhist, st));
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_set_channels_per_wave(ddn_fsk4_rx* b, int channels_per_wave) {
    if (!b || channels_per_wave < 1 || channels_per_wave > 32 || (channels_per_wave & (channels_per_wave - 1))) {
        return DDN_EINVAL;
    }
    b->channels_per_wave = channels_per_wave;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_set_debug_flags(ddn_fsk4_rx* b, int flags) {
    if (!b) {
        return DDN_EINVAL;
    }
    b->dbg_flags = flags;
    return DDN_OK;
}

// per-sync thresholds {center, umid, lmid, max, min} [B][max_syncs][5] (device memory, NULL = off): written by the loop's helper wave
// beside sync_pos / sync_pat; max_syncs = the value the run calls are given
extern "C" int
ddn_fsk4_rx_set_sync_thresholds(ddn_fsk4_rx* b, float* d_thr5) {
    if (!b) {
        return DDN_EINVAL;
    }
    b->dc.sync_thr = d_thr5;
    HIP_TRY(hipMemcpy(b->d_cfg, &b->dc, sizeof(DdnFsk4Config), hipMemcpyHostToDevice));
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_set_timing(ddn_fsk4_rx* b, int enable) {
    if (!b) {
        return DDN_EINVAL;
    }
    if (enable && !b->ev[0]) {
        for (int i = 0; i < 3; i++) {
            HIP_TRY(hipEventCreate(&b->ev[i]));
        }
    }
    b->timing = enable != 0;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_get_timing(ddn_fsk4_rx* b, float* ms2) {
    if (!b || !ms2 || !b->ev[0]) {
        return DDN_EINVAL;
    }
    HIP_TRY(hipEventSynchronize(b->ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms2[0], b->ev[0], b->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms2[1], b->ev[1], b->ev[2]));
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_get_thresholds(ddn_fsk4_rx* b, int channel, float out7[7]) {
    if (!b || !out7 || channel < 0 || channel >= b->cfg.n_channels) {
        return DDN_EINVAL;
    }
    DdnFsk4State s;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&s, b->d_state + channel, sizeof(s), hipMemcpyDeviceToHost));
    out7[0] = s.center;
    out7[1] = s.umid;
    out7[2] = s.lmid;
    out7[3] = s.max;
    out7[4] = s.min;
    out7[5] = s.maxref;
    out7[6] = s.minref;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_rx_run_host(ddn_fsk4_rx* b, const float* disc, size_t n, uint8_t* records10, uint8_t* flags, uint8_t* payload2,
                     int32_t* counts, size_t max_symbols, int32_t* sync_pos, uint8_t* sync_pat, uint8_t* pre, uint8_t* pre_rel,
                     int32_t* n_sync, size_t max_syncs) {
    DDN_TRY(check_fsk4_rx_run(__func__, b, disc, records10, flags, payload2, counts, sync_pos, sync_pat, pre, pre_rel, n_sync));
    const size_t B = (size_t)b->cfg.n_channels, S = B * max_symbols, Y = B * max_syncs;
    DdnStaged s;
    const float* in = s.in(disc, B * n * 4);
    uint8_t* rec = s.out(records10, S * 10);
    uint8_t* fl = s.out(flags, S);
    uint8_t* pay = s.out(payload2, S * 2);
    int32_t* cnt = s.out(counts, B * 4);
    int32_t* spos = s.out(sync_pos, Y * 4);
    uint8_t* spat = s.out(sync_pat, Y);
    uint8_t* p = s.out(pre, Y * DDN_FSK4_PRE);
    uint8_t* pr = s.out(pre_rel, Y * DDN_FSK4_PRE);
    int32_t* ns = s.out(n_sync, B * 4);
    DDN_TRY(s.staged());
    DDN_TRY(ddn_fsk4_rx_run(b, in, n, rec, fl, pay, cnt, max_symbols, spos, spat, p, pr, ns, max_syncs, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    return s.finish();
}

extern "C" int
ddn_dmr_burst_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols, const int32_t* d_sync_pos,
                     const uint8_t* d_pre, const int32_t* d_n_sync, int n_channels, size_t max_syncs, int inverted,
                     uint8_t* d_slot_type, uint8_t* d_info, uint8_t* d_cach, uint8_t* d_valid, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_pre || !d_n_sync || !d_slot_type || !d_info || !d_cach || !d_valid
        || n_channels <= 0) {
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_dmr_burst_gather(d_records10, d_counts, max_symbols, d_sync_pos, nullptr, d_pre, d_n_sync, n_channels, (int)max_syncs,
                                     inverted, d_slot_type, d_info, d_cach, d_valid, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_nxdn_frame_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols, const int32_t* d_sync_pos,
                      const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_lich, uint8_t* d_sacch_sym,
                      uint8_t* d_sacch_rel, uint8_t* d_facch_sym, uint8_t* d_facch_rel, uint8_t* d_valid, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_n_sync || !d_lich || !d_sacch_sym || !d_sacch_rel || !d_facch_sym || !d_facch_rel
        || !d_valid || n_channels <= 0) {
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_nxdn_frame_gather(d_records10, d_counts, max_symbols, d_sync_pos, d_n_sync, n_channels, (int)max_syncs, d_lich,
                                      d_sacch_sym, d_sacch_rel, d_facch_sym, d_facch_rel, d_valid, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_ambe2450_deinterleave_batch(const uint8_t* d_dibits36, const uint8_t* d_reliab36, size_t n, uint8_t* d_ambe_fr,
                                uint8_t* d_ambe_rel, void* hip_stream) {
    if (!d_dibits36 || !d_ambe_fr || (d_ambe_rel && !d_reliab36)) {
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_ambe2450_deinterleave(d_dibits36, d_reliab36, (int)n, d_ambe_fr, d_ambe_rel, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_nxdn_voice_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols, const int32_t* d_sync_pos,
                      const int32_t* d_n_sync, int n_channels, size_t max_syncs, uint8_t* d_ambe_fr, uint8_t* d_ambe_rel,
                      uint8_t* d_valid, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_sync_pos || !d_n_sync || !d_ambe_fr || n_channels <= 0) {
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_nxdn_voice_gather(d_records10, d_counts, max_symbols, d_sync_pos, d_n_sync, (int)max_syncs, n_channels,
                                      d_ambe_fr, d_ambe_rel, d_valid, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_dmr_voice_burst_gather(const uint8_t* d_records10, const int32_t* d_counts, size_t max_symbols,
                           const int32_t* d_burst_start, int n_channels, size_t max_bursts, int inverted, uint8_t* d_ambe_fr,
                           uint8_t* d_ambe_rel, uint8_t* d_sync48, uint8_t* d_cach24, uint8_t* d_valid, void* hip_stream) {
    if (!d_records10 || !d_counts || !d_burst_start || !d_ambe_fr || n_channels <= 0) {
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_dmr_voice_gather(d_records10, d_counts, max_symbols, d_burst_start, (int)max_bursts, n_channels, inverted,
                                     d_ambe_fr, d_ambe_rel, d_sync48, d_cach24, d_valid, (hipStream_t)hip_stream));
    return DDN_OK;
}

extern "C" int
ddn_nxdn_crc_check_batch(const uint8_t* d_bytes, int stride, size_t n, int kind, uint8_t* d_ok, void* hip_stream) {
    if (!d_bytes || !d_ok || stride <= 0 || kind < 0 || kind > 3 || stride * ((kind & 2) ? 1 : 8) < ((kind & 1) == 0 ? 32 : 92)) {
        return DDN_EINVAL;
    }
    HIP_TRY(ddn_dev_nxdn_crc(d_bytes, stride, (int)n, kind, d_ok, (hipStream_t)hip_stream));
    return DDN_OK;
}
