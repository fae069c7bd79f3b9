// ddn_chain_fsk4.h - the fsk4 chain object (include/ddn_chain.h), shared by ddn_api_chain_fsk4.cpp and the mixed chain over it
// (ddn_api_chain_mixed.cpp).  Host code only (not installed).  A common part and one section per protocol; every device buffer is
// allocated through `pool`, which is all that destroy frees.
#ifndef DDN_CHAIN_FSK4_H
#define DDN_CHAIN_FSK4_H

#include "ddn_api_util.h"
#include "ddn_chain.h"
#include "ddn_fsk4.h"
#include "ddn_mbe.h"

struct ddn_fsk4_traits;

struct ddn_fsk4_chain {
    ddn_fsk4_chain_config cfg;
    const ddn_fsk4_traits* tr; // the protocol's row (ddn_api_chain_fsk4.cpp)
    int B, n, T, myc, myd;
    size_t ms, my, stride, S;
    ddn_batch* fe;
    ddn_fsk4_rx* rx;
    DdnPool pool;
    float* d_disc;
    float* d_disc2; // mixed chain only: odd steps' discriminator output (the next call's front end beside this call's loop)
    // (round 6) recorded inside the decode stage once its last reader of the loop's single buffers (sync lists, events) and of the
    // records has been queued: what the NEXT call's loop has to wait for (the frame FEC and the synthesis behind it work on gathered
    // copies) - the mixed chain gates the group's next loop on it instead of on the whole decode stage
    hipEvent_t ev_reads;
    // rows = T carried records + this call's (two sets: the carry reads the previous call's)
    uint8_t *d_rec[2], *d_fl[2], *d_pay;
    int32_t *d_new[2], *d_cnt_full, *d_cnt_scan;
    // what the loop reports per call, the syncs waiting for the next call (two sets), the syncs decoded in this one
    int32_t *s_pos, *s_n, *c_pos[2], *c_n[2], *d_spos, *d_ns, *d_dropped;
    uint8_t *s_pat, *s_pre, *s_prel, *c_pat[2], *c_pre[2], *c_prel[2], *d_spat, *d_pre, *d_prel;
    // the thresholds every sync left, where the protocol's frame decoders read soft symbols (M17, D-STAR, EDACS; NULL otherwise): the
    // loop's list, the carried lists, the decode list
    float *s_thr, *c_thr[2], *d_thr;
    // the AMBE 3600x2450 voice tail of the protocols with vocoder = 1: the vocoder batch (NULL = no voice), the frames filed by talk
    // path (V slots: DMR bursts, NXDN frames), their count per path, frame FEC in / out, the frames to skip, PCM, the synthesis' result
    ddn_mbe_batch* mbe;
    size_t V;
    int32_t *d_vn, *d_ambe_res, *d_res_out;
    uint8_t *d_ambe_fr, *d_ambe_rel, *d_ambe_d, *d_skip;
    float* d_pcm;

    struct {
        uint8_t *st, *info, *cach, *valid, *st_ok, *pdu, *r3;
        uint32_t* errs;
        // voice (vocoder = 1): the loop's handler decisions of the call, the voice bursts they name filed by talk path (2 per
        // channel: time slots 1 / 2), three AMBE frames each
        int E, vb;
        int32_t *ev, *nev, *vstart, *vpre, *vnb;
        // data bursts the handlers dispatch (handlers = 1): db per channel and call, D = B * db; embedded link control: lb per talk
        // path and call, L = 2 B * lb (ddn_dmr_data.hip)
        int db, lb;
        size_t D, L;
        struct {
            int32_t *start, *pre, *n, *listn, *pooln;
            uint32_t* errs;
            uint8_t *slot, *st, *st_ok, *info, *td, *rel, *pdu, *r3, *type, *bytes, *cw, *rsres, *rsfound, *crc, *want, *hard, *soft, *list,
                *backs, *pool, *unconf, *conf, *confcrc;
        } data;
        struct {
            int32_t *pos, *n;
            uint32_t* errs;
            uint8_t *sig, *in, *out, *ok;
        } emb;
        // data PDUs (ddn_dmr_pdu.hip), off until ddn_fsk4_chain_set_dmr_pdu_slots: P = 0, nothing allocated, nothing launched.  The
        // state carried per channel, the marks of a call (M per channel), the walk's outputs per burst and - P slots per channel, made
        // at the first run - per completed PDU
        struct {
            int P, M;
            uint8_t *state, *b_conf, *b_crc, *b_dbsn, *b_status, *kind, *slot, *bytes, *crc4, *bcrc;
            int32_t *b_counter, *b_pick, *n_pdus, *burst, *len, *hdr, *rb, *nr, *lb, *nl;
        } pw;
        // MS / direct-mode bursts (ddn_dmr_ms.hip), off until ddn_fsk4_chain_set_dmr_ms: nothing allocated, nothing launched.  The state
        // carried per channel, the walk's lists and the decoders' outputs (include/ddn_fsk4.h), a vocoder batch of B talk paths
        struct {
            int on;
            uint8_t* state;
            ddn_dmr_ms_bursts b;
            ddn_dmr_ms_data d;
            ddn_dmr_ms_voice v;
            ddn_mbe_batch* mbe;
        } ms;
    } dmr;
    struct { // NXDN48 / NXDN96; vf: voice frames per channel and call
        int vf;
        uint8_t *lich, *valid, *ss, *sr, *fs, *fr, *sacch, *sacch_ok, *hard_in, *sacch_hard, *sacch_hard_ok, *facch, *facch_ok;
        int32_t* vpos;
        // CAC / FACCH2 / UDCH frames and the SACCH walk (ddn_nxdn_ctrl.hip), off until ddn_fsk4_chain_set_nxdn_ctrl: nothing allocated,
        // nothing launched.  The state carried per channel, the outputs per sync slot
        struct {
            int on;
            uint8_t *state, *kind, *bits, *bytes, *crc, *fallback, *ran, *sf, *sacch_status, *pf, *seq, *msg, *msg_status;
            int32_t *last_ran, *cac_fail;
        } ctrl;
    } nxdn;
    struct { // M17: the frame decoders' slot arrays (ddn_m17_*_batch), the carried LICH assembly buffer
        uint8_t *lsf, *lsf_st, *l6, *cnt, *fp, *st, *assembly, *ll, *ll_st;
        uint32_t* cost;
        // packet and BERT frames (ddn_m17_data.hip): the frame decoders' slot arrays, the state carried per channel, the walk's outputs
        // per sync slot and - P slots per channel, made at the first run - per completed packet
        int P;
        uint8_t *p26, *pf_st, *b25, *bf_st, *data_state, *p_st, *p_cnt, *packet, *packet_ok;
        uint32_t* p_cost;
        int32_t *b_state, *n_packets, *packet_len, *packet_slot;
    } m17;
    struct { // YSF: the frame information channel of every decoded sync
        uint8_t *fich4, *st;
        uint32_t* ve;
        // ... and the payload behind it (ddn_ysf_payload_decode_batch): the frame type carried per channel, the data channels, V/D2 voice bits
        uint8_t *last, *info, *dch, *dst, *ambe, *errs, *fr, *nfr;
        uint32_t* dcost;
        // ... V/D mode 2 voice (vocoder = 1): the sub-frames filed by talk path (= channel) -> the AMBE voice tail (vf frames of five
        // sub-frames per channel and call)
        int vf;
        int32_t* vslot;
        // ... V/D mode 1 (four AMBE frames through the frame FEC, filed with the V/D mode 2 sub-frames in stream order) and full-rate voice
        // (IMBE 7200x4400: a vocoder batch, talk-path history and PCM of its own)
        ddn_mbe_batch* mbe_i;
        uint8_t *f96, *b49, *b88, *i_bits, *i_skip;
        int32_t *r49, *r88, *i_res, *i_res_out, *i_vn, *i_vslot;
        float* i_pcm;
    } ysf;
    // dPMR: the superframe behind every decoded sync (ddn_dpmr.hip), the identity state per channel, and with vocoder = 1 the eight TCH
    // frames per slot, the voiced halves filed by channel (vf frames each) -> the AMBE voice tail
    struct {
        int vf;
        uint8_t *bits, *ham, *crc, *valid, *kind, *strong, *fr, *voiced, *muted, *vfr, *vhalf, *vmuted;
        int32_t *fields, *id, *color, *tg, *src, *state, *vslot;
    } dpmr;
    struct { // D-STAR: the radio header and the voice superframe behind every decoded sync (ddn_dstar.hip), read against d_thr
        uint8_t *h41, *hok, *hv, *ambe, *sdb, *kind, *sh41, *sok, *text, *vv;
    } dstar;
    // EDACS: the control-channel frame behind every decoded sync (ddn_edacs.hip), read against d_thr, under the mode
    // ddn_fsk4_chain_set_edacs_mode selects
    struct {
        int ea_mode, esk_mask;
        uint64_t *raw, *vote;
        uint32_t* msg;
        int32_t* site;
        uint8_t *bok, *fok, *kind, *types, *valid;
    } edacs;
    long step;
    int last_set;
};

#endif
