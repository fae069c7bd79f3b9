/*
 * tests/edacs_rx.c - TEST INFRASTRUCTURE ONLY: CPU restatement of the receive loop on the 9600_2 hunt profile (EDACS, -fh / -fH / -fe /
 * -fE), between the discriminator stream and the records, for the comparison with DDN_FSK4_EDACS (tests/test_edacs_gpu.py).  The oracle
 * loop (oracle/ddn_oracle_rx4.c) holds a 24-symbol sign history and 32-bit patterns; this one is the same loop restated for 48-symbol
 * words from the reference, not from the kernel:
 *
 *   getSymbol() RTL-FSK path    src/dsp/dsd_symbol.c:1343-1387,1769-1805 at 5 samples per symbol: accumulation :404-460 (the
 *                               5-sample symbol adds samples 1, 2 and 3 - the centre through its own rule, the GFSK edges l = r = 1
 *                               through select_window_gfsk() :197-224; C4FM 0..4 through the C4FM window), slip rules :462-517,
 *                               in-sync clip on C4FM only :347-358, no matched filter (symbol_apply_matched_filter() :300-336)
 *   getFrameSync()              src/dsp/dsd_frame_sync.c:3098-3148; ring :1729-1764 (level ring 24, frame_sync_select_t_max()
 *                               default branch); sign history :2250-2310 (48-symbol window materialised once 48 symbols are in);
 *                               level window from 8 symbols on; timeouts :2753-2760,3037-3053
 *     EDACS accept              frame_sync_try_provoice() :1421-1450 (EDACS_SYNC exact -> DSD_SYNC_EDACS_NEG, INV_EDACS_SYNC exact ->
 *                               DSD_SYNC_EDACS_POS), frame_sync_accept_edacs() :1399-1409: basic lock :385-392 and
 *                               dsd_sync_warm_start_thresholds_outer_only(opts, state, 48)
 *   in-frame symbol             get_dibit_and_analog_signal, src/core/frames/dsd_dibit.c:1045-1076; thresholds static (use_symbol()
 *                               :261-275); edacs() reads 240 symbols (edacs-fme.c:1966-1970)
 *
 * The records are written as the oracle loop writes them (four-level slice + reliability in frame, the sign while hunting), so the
 * comparison reuses its helpers from oracle/libddn_oracle.so: the slicer, the reliability, the level estimate, the warm start, the
 * slip rule and the window.  The ProVoice words the same reference hunt compares are not hunted (include/ddn_fsk4.h).
 */
#include <string.h>

#include "ddn_oracle.h"

#define EDRX_HIST 96
#define EDRX_WIN 48
#define EDRX_TMAX 24

typedef struct edrx {
    int out_rate, rf_mod, lock_symbols;
    uint64_t pat[2];
    orc_slicer sl;
    int need_reset, sps_accum, jitter, span, centre, i, count, in_symbol;
    float sum, lastsample;
    int have_sync, lock_left, lastsync, cur_pat;
    float lbuf[EDRX_TMAX];
    int lidx, level_count, hist_count, hunt_pos;
    uint64_t hist_bits;
    float lmin, lmax;
    float shist[EDRX_HIST];
    uint8_t phist[EDRX_HIST], rhist[EDRX_HIST];
    int shead, scount;
    long n_sym;
    float* sync_thr;
    int sync_thr_max, sync_thr_n;
} edrx;

static uint64_t
word_bits(const char* s) {
    uint64_t v = 0;
    for (; *s; s++) {
        v = (v << 1) | (*s == '1' ? 1u : 0u);
    }
    return v;
}

size_t
edrx_sizeof(void) {
    return sizeof(edrx);
}

/* words: EDACS_SYNC then INV_EDACS_SYNC as '1' / '3' strings (tests/golden/edacs_vectors.json) */
void
edrx_init(edrx* r, int out_rate, int rf_mod, int lock_symbols, const char* word0, const char* word1) {
    memset(r, 0, sizeof(*r));
    r->out_rate = out_rate;
    r->rf_mod = rf_mod;
    r->lock_symbols = lock_symbols;
    r->pat[0] = word_bits(word0);
    r->pat[1] = word_bits(word1);
    r->jitter = -1;
    orc_slicer_init(&r->sl, 0);
    r->lmin = r->sl.min;
    r->lmax = r->sl.max;
}

static void
no_carrier(edrx* r) {
    r->jitter = -1;
    r->lastsync = 0;
    r->sl.max = 15000.0f;
    r->sl.min = -15000.0f;
    r->sl.center = 0.0f;
    r->need_reset = 1;
}

static void
hunt_enter(edrx* r) {
    r->hunt_pos = 0;
    r->have_sync = 0;
    r->lidx = 0;
    r->level_count = 0;
    r->hist_count = 0;
    r->hist_bits = 0;
    r->lmin = r->sl.min;
    r->lmax = r->sl.max;
}

static void
symbol_begin(edrx* r) {
    if (r->need_reset) {
        orc_slicer* s = &r->sl;
        r->need_reset = 0;
        r->sps_accum = 0;
        r->jitter = -1;
        s->center = 0.0f;
        s->min = -30000.0f;
        s->max = 30000.0f;
        s->lmid = -20000.0f;
        s->umid = 20000.0f;
        s->minref = -24000.0f;
        s->maxref = 24000.0f;
        for (int i = 0; i < ORC_SLICER_MSIZE; i++) {
            s->minbuf[i] = s->min;
            s->maxbuf[i] = s->max;
        }
        s->midx = 0;
        s->sums_valid = 0;
    }
    const int sps = r->out_rate / 9600; /* (the host admits 9600 x 5..10 only: no remainder) */
    r->span = sps;
    r->centre = (sps - 1) / 2;
    r->sum = 0.0f;
    r->count = 0;
    r->in_symbol = 1;
    r->i = orc_fsk4_adjust_timing(sps, r->centre, r->rf_mod, r->jitter, r->have_sync, sps, 0, &r->jitter);
}

static void
sample_step(edrx* r, float x) {
    orc_slicer* s = &r->sl;
    if (r->have_sync && r->rf_mod == 0) {
        x = x > s->max ? s->max : (x < s->min ? s->min : x);
    }
    const int i = r->i, c = r->centre;
    if (x > s->center) {
        if (!(x > s->maxref * 1.25f) && r->jitter < 0 && r->lastsample < s->center) {
            r->jitter = i;
        }
    } else {
        if (!(x < s->minref * 1.25f) && r->jitter < 0 && r->lastsample > s->center) {
            r->jitter = i;
        }
    }
    int take;
    if (r->span == 5 && i == 2) {
        take = 1;
    } else {
        int l, rr;
        orc_fsk4_window(r->rf_mod, 0, &l, &rr);
        take = r->rf_mod == 0 ? (i >= c - l && i <= c + rr) : (r->span <= 4 ? i == c : (i == c - l || i == c + rr));
    }
    if (r->span == 20 && i >= 7 && i <= 13) {
        r->sum += x;
        r->count++;
    }
    if (take) {
        r->sum += x;
        r->count++;
    }
    r->lastsample = x;
    r->i++;
}

static int
slice4(const orc_slicer* s, float sym) {
    if (sym > s->center) {
        return (sym > s->umid) ? 1 : 0;
    }
    return (sym < s->lmid) ? 3 : 2;
}

static void
sort_small(float* v, int n) {
    for (int i = 1; i < n; i++) {
        const float x = v[i];
        int j = i - 1;
        while (j >= 0 && v[j] > x) {
            v[j + 1] = v[j];
            j--;
        }
        v[j + 1] = x;
    }
}

static int
symbol_commit(edrx* r, float sym, int rec4[4], uint8_t pay2[2]) {
    orc_slicer* s = &r->sl;
    const int slot = r->shead;
    r->shist[slot] = sym;
    r->shead = (r->shead + 1) % EDRX_HIST;
    if (r->scount < EDRX_HIST) {
        r->scount++;
    }
    if (r->have_sync) {
        const int neg = r->cur_pat == 0; /* EDACS_SYNC = -EDACS */
        s->negative = neg;
        orc_slicer_step_static(s, sym, rec4);
        const int d = rec4[0];
        pay2[0] = (uint8_t)(neg ? (d ^ 2) : d);
        pay2[1] = (uint8_t)rec4[1];
        r->phist[slot] = pay2[0];
        r->rhist[slot] = pay2[1];
        if (--r->lock_left <= 0) {
            hunt_enter(r);
        }
        return 1 | (neg ? 4 : 0);
    }
    r->lbuf[r->lidx] = sym;
    if (r->level_count < EDRX_TMAX) {
        r->level_count++;
    }
    s->sbuf[s->sidx] = sym;
    r->lidx = (r->lidx == EDRX_TMAX - 1) ? 0 : r->lidx + 1;
    s->sidx = (s->sidx == ORC_SLICER_SSIZE - 1) ? 0 : s->sidx + 1;
    const int bit = sym > 0 ? 1 : 0;
    r->hist_bits = ((r->hist_bits << 1) | (uint64_t)bit) & ((1ull << EDRX_WIN) - 1ull);
    if (r->hist_count < EDRX_WIN) {
        r->hist_count++;
    }
    rec4[0] = bit ? 1 : 3;
    rec4[1] = rec4[2] = rec4[3] = 0;
    pay2[0] = (uint8_t)slice4(s, sym);
    pay2[1] = (uint8_t)orc_slicer_reliability(s, sym);
    r->phist[slot] = pay2[0];
    r->rhist[slot] = pay2[1];
    if (r->hist_count >= 8) {
        float tmp[EDRX_TMAX];
        memcpy(tmp, r->lbuf, sizeof(float) * (size_t)r->level_count);
        sort_small(tmp, r->level_count);
        orc_level_estimate(tmp, r->level_count, &r->lmin, &r->lmax);
        s->maxref = s->max;
        s->minref = s->min;
        int hit = -1;
        if (r->hist_count >= EDRX_WIN) {
            hit = r->hist_bits == r->pat[0] ? 0 : (r->hist_bits == r->pat[1] ? 1 : -1);
        }
        if (hit >= 0) {
            s->max = (s->max + r->lmax) / 2;
            s->min = (s->min + r->lmin) / 2;
            r->lastsync = hit == 0 ? 39 : 38;
            if (r->scount >= EDRX_WIN) {
                float nf[EDRX_WIN];
                for (int k = 0; k < EDRX_WIN; k++) {
                    nf[k] = r->shist[(r->shead - 1 - k + 4 * EDRX_HIST) % EDRX_HIST];
                }
                (void)orc_slicer_warm_start(s, nf, EDRX_WIN);
            }
            if (r->sync_thr && r->sync_thr_n < r->sync_thr_max) {
                float* t = r->sync_thr + 5 * (size_t)r->sync_thr_n;
                t[0] = s->center, t[1] = s->umid, t[2] = s->lmid, t[3] = s->max, t[4] = s->min;
            }
            r->sync_thr_n++;
            r->have_sync = 1;
            r->cur_pat = hit;
            r->lock_left = r->lock_symbols;
            if (r->lock_left <= 0) {
                hunt_enter(r);
            }
            return 2 | (hit == 0 ? 4 : 0) | (hit << 3);
        }
    }
    if (r->hunt_pos < 10200) {
        r->hunt_pos++;
    } else {
        r->hunt_pos = 0;
        no_carrier(r);
    }
    if (r->hunt_pos >= 1800) {
        no_carrier(r);
        hunt_enter(r);
    }
    return 0;
}

/* the outputs of orc_fsk4rx_run() (oracle/ddn_oracle_rx4.c), pre / pre_rel = the 90 payload dibits ending at a sync */
long
edrx_run(edrx* r, const float* in, long n, float* out_sym, int* rec4, uint8_t* flags, uint8_t* pay2, long max_out, int32_t* sync_pos,
         uint8_t* sync_pat, uint8_t* pre, uint8_t* pre_rel, int max_sync, int* n_sync) {
    long o = 0;
    int ns = 0;
    for (long k = 0; k < n; k++) {
        if (!r->in_symbol) {
            symbol_begin(r);
        }
        sample_step(r, in[k]);
        if (r->i >= r->span) {
            const float sym = (r->count > 0) ? (r->sum / (float)r->count) : 0.0f;
            r->in_symbol = 0;
            int rr[4];
            uint8_t pp[2];
            const int f = symbol_commit(r, sym, rr, pp);
            r->n_sym++;
            if (o < max_out) {
                out_sym[o] = sym;
                memcpy(rec4 + 4 * o, rr, sizeof(rr));
                flags[o] = (uint8_t)f;
                pay2[2 * o] = pp[0];
                pay2[2 * o + 1] = pp[1];
            }
            if (f & 2) {
                if (ns < max_sync) {
                    sync_pos[ns] = (int32_t)o;
                    sync_pat[ns] = (uint8_t)((f >> 3) & 31);
                    for (int i = 0; i < 90; i++) {
                        const int sl = (r->shead - 90 + i + 4 * EDRX_HIST) % EDRX_HIST;
                        const int have = (90 - i) <= r->scount;
                        pre[(size_t)ns * 90 + i] = have ? r->phist[sl] : 0;
                        pre_rel[(size_t)ns * 90 + i] = have ? r->rhist[sl] : 0;
                    }
                }
                ns++;
            }
            o++;
        }
    }
    *n_sync = ns;
    return o;
}

void
edrx_set_sync_thresholds(edrx* r, float* buf, int max_syncs) {
    r->sync_thr = buf;
    r->sync_thr_max = max_syncs;
    r->sync_thr_n = 0;
}

void
edrx_get_thresholds(const edrx* r, float out7[7]) {
    out7[0] = r->sl.center;
    out7[1] = r->sl.umid;
    out7[2] = r->sl.lmid;
    out7[3] = r->sl.max;
    out7[4] = r->sl.min;
    out7[5] = r->sl.maxref;
    out7[6] = r->sl.minref;
}
