// ddn_api_chain_fsk4.cpp - the chain object of the protocols behind the fsk4 receive loop (include/ddn_chain.h): stage order, buffers
// and streams on top of the library's own C-ABI stage calls.  Host-only code.  A protocol is its row of the loop's table
// (ddn_fsk4::kRow, ddn_fsk4_proto.h), a row of fsk4_traits[], a section of ddn_fsk4_chain (ddn_chain_fsk4.h), a <proto>_alloc and a
// <proto>_decode.
//
// What it stands in for in a dsd-neo host: the demodulator thread's per-block loop (src/io/radio/rtl_sdr_fm.cpp:3458-3516) and
// processFrame()'s DMR / NXDN branches (src/engine/protocol_dispatch.c -> dmr_data.c / dmr_bs.c, nxdn_frame.c), B channels wide.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "ddn_chain_fsk4.h"
#include "ddn_device.h"
#include "ddn_fsk4_proto.h"
#include "ddn_hip.h"

struct ddn_fsk4_traits {
    int levels, lpf;           // the front end: slicer levels, channel filter (its symbols/s are the loop's, ddn_fsk4::kRow)
    int T;                     // the tail of records kept back for the next call: a frame that began in this call ends inside it
    int min_sync_gap;          // symbols between two accepted syncs at least: bounds the decode slots (0 = the general bound)
    bool thresholds;           // every sync files the thresholds it left (s_thr / c_thr / d_thr)
    // what the configuration may ask for: inverted up to this value (-1 = not looked at), the vocoder, an rf_mod other than 0 / 2
    // (the handlers in the loop: where the loop's row has a handler family)
    int inverted_max;
    bool vocoder, any_rf_mod;
    int (*alloc)(ddn_fsk4_chain*);
    int (*decode)(ddn_fsk4_chain*, int cur, int flush, hipStream_t);
};

// a zero-filled device buffer of the chain, freed with it
#define BUF(field, count) c->pool.alloc(&c->field, (count))

static int
alloc_rc(bool ok) {
    if (!ok) {
        ddn_set_error("ddn_fsk4_chain_create: device allocation failed");
    }
    return ok ? DDN_OK : DDN_ENOMEM;
}

// the AMBE voice tail behind `frames` filed frames (the caller allocates what files them)
static int
voice_tail_alloc(ddn_fsk4_chain* c, size_t frames, int talk_paths) {
    DDN_TRY(alloc_rc(BUF(d_ambe_d, frames * 49) && BUF(d_ambe_res, frames * 5) && BUF(d_skip, frames) && BUF(d_pcm, frames * 160)
                       && BUF(d_res_out, frames * 5)));
    return ddn_mbe_batch_create(DDN_MBE_AMBE_3600X2450, talk_paths, &c->mbe);
}

// ---- YSF ----------------------------------------------------------------------------------------------------------------------------
static int
ysf_alloc(ddn_fsk4_chain* c) {
    const size_t B = (size_t)c->B, S = c->S;
    DDN_TRY(alloc_rc(BUF(ysf.fich4, S * 4) && BUF(ysf.st, S) && BUF(ysf.ve, S) && BUF(ysf.last, B * 2) && BUF(ysf.info, S * 2)
                       && BUF(ysf.dch, S * 40) && BUF(ysf.dst, S * 2) && BUF(ysf.dcost, S * 2) && BUF(ysf.ambe, S * 5 * 49)
                       && BUF(ysf.errs, S * 5) && BUF(ysf.fr, S * 5 * 184) && BUF(ysf.nfr, S)));
    if (!c->cfg.vocoder) {
        return DDN_OK;
    }
    c->ysf.vf = (int)(c->stride / 480 + 2);
    const size_t V5 = B * (size_t)c->ysf.vf * 5;
    DDN_TRY(alloc_rc(BUF(ysf.vslot, B * (size_t)c->ysf.vf) && BUF(d_vn, B) && BUF(ysf.f96, S * 5 * 96) && BUF(ysf.b49, S * 5 * 49)
                       && BUF(ysf.r49, S * 5 * 5) && BUF(ysf.b88, S * 5 * 88) && BUF(ysf.r88, S * 5 * 5) && BUF(ysf.i_bits, V5 * 88)
                       && BUF(ysf.i_res, V5 * 5) && BUF(ysf.i_res_out, V5 * 5) && BUF(ysf.i_skip, V5) && BUF(ysf.i_pcm, V5 * 160)
                       && BUF(ysf.i_vn, B) && BUF(ysf.i_vslot, B * (size_t)c->ysf.vf)));
    DDN_TRY(voice_tail_alloc(c, V5, c->B));
    return ddn_mbe_batch_create(DDN_MBE_IMBE_7200X4400, c->B, &c->ysf.mbe_i);
}

static int
ysf_decode(ddn_fsk4_chain* c, int cur, int, hipStream_t st) {
    const uint8_t* rec = c->d_rec[cur];
    // the frame information channel behind every sync of the decode list (row a17's second consumer)
    DDN_TRY(ddn_ysf_fich_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_ns, c->B, (size_t)c->myd, c->ysf.fich4, c->ysf.st, c->ysf.ve, st));
    // ... and the payload of every frame: V/D mode 2 voice bits + DCH2, the DCH blocks of V/D mode 1 and of the full-rate data frames
    DDN_TRY(ddn_ysf_payload_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_ns, c->B, (size_t)c->myd, c->ysf.fich4, c->ysf.st,
                                         c->ysf.last, c->ysf.info, c->ysf.dch, c->ysf.dst, c->ysf.dcost, c->ysf.ambe, c->ysf.errs, c->ysf.fr, c->ysf.nfr, st));
    if (c->mbe) { // mbe_processAmbe2450Dataf of every V/D mode 2 sub-frame, talk path = channel (ysf_handle_vd_type2, ysf.c:753-755)
        // the frames of V/D mode 1 and of full-rate voice through the frame FEC (processMbeFrame's hard decode, dsd_mbe.c:54-92), slot by slot
        const size_t S5 = c->S * 5, V5 = (size_t)c->B * (size_t)c->ysf.vf * 5;
        HIP_TRY(ddn_dev_ysf_pack96(c->ysf.fr, S5, c->ysf.f96, st));
        DDN_TRY(ddn_mbe_frame_decode_batch(DDN_MBE_AMBE_3600X2450, c->ysf.f96, nullptr, S5, c->ysf.b49, c->ysf.r49, st));
        DDN_TRY(ddn_mbe_frame_decode_batch(DDN_MBE_IMBE_7200X4400, c->ysf.fr, nullptr, S5, c->ysf.b88, c->ysf.r88, st));
        HIP_TRY(ddn_dev_ysf_voice_file(c->d_ns, c->B, c->myd, c->ysf.info, c->ysf.ambe, c->ysf.errs, c->ysf.b49, c->ysf.r49, c->ysf.nfr, 0, c->ysf.vf,
                                       c->d_ambe_d, c->d_ambe_res, c->d_skip, c->d_vn, c->ysf.vslot, st));
        DDN_TRY(ddn_mbe_result_skip_batch(c->d_skip, V5, c->d_ambe_res, st));
        DDN_TRY(ddn_mbe_synth_batch(c->mbe, c->d_ambe_d, c->d_ambe_res, (size_t)c->ysf.vf * 5, c->d_pcm, c->d_res_out, st));
        HIP_TRY(ddn_dev_ysf_voice_file(c->d_ns, c->B, c->myd, c->ysf.info, c->ysf.ambe, c->ysf.errs, c->ysf.b88, c->ysf.r88, c->ysf.nfr, 1, c->ysf.vf,
                                       c->ysf.i_bits, c->ysf.i_res, c->ysf.i_skip, c->ysf.i_vn, c->ysf.i_vslot, st));
        DDN_TRY(ddn_mbe_result_skip_batch(c->ysf.i_skip, V5, c->ysf.i_res, st));
        DDN_TRY(ddn_mbe_synth_batch(c->ysf.mbe_i, c->ysf.i_bits, c->ysf.i_res, (size_t)c->ysf.vf * 5, c->ysf.i_pcm, c->ysf.i_res_out, st));
    }
    HIP_TRY(hipEventRecord(c->ev_reads, st));
    return DDN_OK;
}

// ---- EDACS --------------------------------------------------------------------------------------------------------------------------
static int
edacs_alloc(ddn_fsk4_chain* c) {
    const size_t S = c->S;
    return alloc_rc(BUF(edacs.raw, S * 6) && BUF(edacs.vote, S * 2) && BUF(edacs.msg, S * 2) && BUF(edacs.site, S * 6) && BUF(edacs.bok, S * 2)
                      && BUF(edacs.fok, S) && BUF(edacs.kind, S) && BUF(edacs.types, S * 3) && BUF(edacs.valid, S));
}

static int
edacs_decode(ddn_fsk4_chain* c, int cur, int, hipStream_t st) {
    // every frame of the decode list (each whole inside the row): bits, vote, BCH re-encode, ESK, message types, site ID
    DDN_TRY(ddn_edacs_frame_decode_batch(c->d_rec[cur], c->stride, c->d_cnt_full, c->d_spos, c->d_spat, c->d_ns, c->d_thr, c->B, (size_t)c->myd,
                                         c->edacs.ea_mode, c->edacs.esk_mask, c->edacs.raw, c->edacs.vote, c->edacs.bok, c->edacs.fok, c->edacs.msg,
                                         c->edacs.kind, c->edacs.types, c->edacs.site, c->edacs.valid, st));
    HIP_TRY(hipEventRecord(c->ev_reads, st));
    return DDN_OK;
}

// ---- D-STAR -------------------------------------------------------------------------------------------------------------------------
static int
dstar_alloc(ddn_fsk4_chain* c) {
    const size_t S = c->S;
    return alloc_rc(BUF(dstar.h41, S * 41) && BUF(dstar.hok, S) && BUF(dstar.hv, S) && BUF(dstar.ambe, S * 21 * 96) && BUF(dstar.sdb, S * 60)
                      && BUF(dstar.kind, S) && BUF(dstar.sh41, S * 41) && BUF(dstar.sok, S) && BUF(dstar.text, S * 60) && BUF(dstar.vv, S));
}

static int
dstar_decode(ddn_fsk4_chain* c, int cur, int, hipStream_t st) {
    const uint8_t* rec = c->d_rec[cur];
    // every unit of the decode list (each whole inside the row): the radio header behind a header sync, the voice superframe and
    // its slow data behind every sync
    DDN_TRY(ddn_dstar_header_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_spat, c->d_ns, c->d_thr, c->B, (size_t)c->myd,
                                          c->dstar.h41, c->dstar.hok, c->dstar.hv, st));
    DDN_TRY(ddn_dstar_voice_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_spat, c->d_ns, c->d_thr, c->B, (size_t)c->myd,
                                         c->dstar.ambe, c->dstar.sdb, c->dstar.kind, c->dstar.sh41, c->dstar.sok, c->dstar.text, c->dstar.vv, st));
    HIP_TRY(hipEventRecord(c->ev_reads, st));
    return DDN_OK;
}

// ---- dPMR ---------------------------------------------------------------------------------------------------------------------------
static int
dpmr_alloc(ddn_fsk4_chain* c) {
    const size_t B = (size_t)c->B, S = c->S;
    DDN_TRY(alloc_rc(BUF(dpmr.bits, S * 96) && BUF(dpmr.ham, S * 12) && BUF(dpmr.crc, S * 2) && BUF(dpmr.fields, S * 16) && BUF(dpmr.id, S)
                       && BUF(dpmr.color, S) && BUF(dpmr.valid, S) && BUF(dpmr.kind, S) && BUF(dpmr.strong, S) && BUF(dpmr.tg, S)
                       && BUF(dpmr.src, S) && BUF(dpmr.state, B * 3)));
    { // {tg, src, next part} = {none, none, 0}
        int32_t* h = new (std::nothrow) int32_t[B * 3];
        bool ok = h != nullptr;
        for (size_t i = 0; ok && i < B; i++) {
            h[3 * i] = -1, h[3 * i + 1] = -1, h[3 * i + 2] = 0;
        }
        ok = ok && hipMemcpy(c->dpmr.state, h, sizeof(int32_t) * B * 3, hipMemcpyHostToDevice) == hipSuccess;
        delete[] h;
        DDN_TRY(alloc_rc(ok));
    }
    if (!c->cfg.vocoder) {
        return DDN_OK;
    }
    // two halves of four frames per superframe; the superframes a call decodes: see myd (a carried one included)
    c->dpmr.vf = 8 * (int)(c->ms / 384 + 2);
    const size_t V = B * (size_t)c->dpmr.vf;
    DDN_TRY(alloc_rc(BUF(dpmr.fr, S * 8 * 96) && BUF(dpmr.voiced, S * 2) && BUF(dpmr.muted, S * 2) && BUF(dpmr.vfr, V * 96) && BUF(dpmr.vslot, V)
                       && BUF(dpmr.vhalf, V) && BUF(dpmr.vmuted, V) && BUF(d_vn, B)));
    return voice_tail_alloc(c, V, c->B);
}

static int
dpmr_decode(ddn_fsk4_chain* c, int cur, int, hipStream_t st) {
    const uint8_t* rec = c->d_rec[cur];
    // every superframe of the decode list (each whole inside the row): CCHs, colour code, ID -> the identity rules in sync order
    DDN_TRY(ddn_dpmr_superframe_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_ns, c->B, (size_t)c->myd, c->cfg.inverted,
                                             c->dpmr.bits, c->dpmr.ham, c->dpmr.crc, c->dpmr.fields, c->dpmr.id, c->dpmr.color, c->dpmr.valid, st));
    if (c->mbe) {
        DDN_TRY(ddn_dpmr_voice_gather(rec, c->stride, c->d_spos, c->d_ns, c->B, (size_t)c->myd, c->cfg.inverted, c->dpmr.fields, c->dpmr.valid,
                                      c->dpmr.fr, c->dpmr.voiced, c->dpmr.muted, st));
    }
    HIP_TRY(hipEventRecord(c->ev_reads, st)); // (everything below works on the decoded fields and the gathered frames)
    DDN_TRY(ddn_dpmr_identity_batch(c->d_ns, c->B, (size_t)c->myd, c->dpmr.valid, c->dpmr.fields, c->dpmr.ham, c->dpmr.crc, c->dpmr.id, c->dpmr.state,
                                    c->dpmr.kind, c->dpmr.strong, c->dpmr.tg, c->dpmr.src, st));
    if (c->mbe) {
        // voice (dpmr_play_voice_frames): the voiced halves in air order, talk path = channel -> frame FEC (hard bits) -> synthesis
        const size_t V = (size_t)c->B * (size_t)c->dpmr.vf;
        HIP_TRY(ddn_dev_dpmr_voice_file(c->d_ns, c->B, c->myd, c->dpmr.fr, c->dpmr.voiced, c->dpmr.muted, c->dpmr.vf, c->dpmr.vfr, c->d_vn, c->dpmr.vslot,
                                        c->dpmr.vhalf, c->dpmr.vmuted, c->d_skip, st));
        DDN_TRY(ddn_mbe_frame_decode_batch(DDN_MBE_AMBE_3600X2450, c->dpmr.vfr, nullptr, V, c->d_ambe_d, c->d_ambe_res, st));
        DDN_TRY(ddn_mbe_result_skip_batch(c->d_skip, V, c->d_ambe_res, st));
        DDN_TRY(ddn_mbe_synth_batch(c->mbe, c->d_ambe_d, c->d_ambe_res, (size_t)c->dpmr.vf, c->d_pcm, c->d_res_out, st));
    }
    return DDN_OK;
}

// ---- M17 ----------------------------------------------------------------------------------------------------------------------------
static int
m17_alloc(ddn_fsk4_chain* c) {
    const size_t S = c->S;
    return alloc_rc(BUF(m17.lsf, S * 30) && BUF(m17.lsf_st, S) && BUF(m17.l6, S * 6) && BUF(m17.cnt, S) && BUF(m17.fp, S * 18) && BUF(m17.st, S)
                      && BUF(m17.assembly, (size_t)c->B * 32) && BUF(m17.ll, S * 30) && BUF(m17.ll_st, S) && BUF(m17.cost, S)
                      // packet and BERT frames; the carried state starts all zeros (= a stream's start)
                      && BUF(m17.p26, S * 26) && BUF(m17.pf_st, S) && BUF(m17.p_cost, S) && BUF(m17.b25, S * 25) && BUF(m17.bf_st, S)
                      && BUF(m17.data_state, (size_t)c->B * ddn_m17_data_state_bytes()) && BUF(m17.p_st, S) && BUF(m17.p_cnt, S)
                      && BUF(m17.b_state, S * 8) && BUF(m17.n_packets, (size_t)c->B));
}

static int
m17_decode(ddn_fsk4_chain* c, int cur, int, hipStream_t st) {
    const uint8_t* rec = c->d_rec[cur];
    // the frames behind the syncs of this call's decode list (each complete inside the row): link setup frames through the K = 5
    // decoder of row a17, stream frames (LICH + payload), the LSF reassembled from the LICH chunks across calls
    DDN_TRY(ddn_m17_lsf_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_spat, c->d_ns, c->d_thr, c->B, (size_t)c->myd, c->m17.lsf,
                                     c->m17.lsf_st, c->m17.cost, st));
    DDN_TRY(ddn_m17_str_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_spat, c->d_ns, c->B, (size_t)c->myd, c->m17.l6, c->m17.cnt,
                                     c->m17.fp, c->m17.st, st));
    DDN_TRY(ddn_m17_lich_assemble_batch(c->d_spat, c->d_ns, c->B, (size_t)c->myd, c->m17.lsf, c->m17.lsf_st, c->m17.l6, c->m17.cnt, c->m17.st,
                                        c->m17.assembly, c->m17.ll, c->m17.ll_st, st));
    // packet and BERT frames, then the walk that carries a packet and the BERT receiver across calls (this call's new records are
    // what the next call's rows begin behind)
    if (!c->m17.packet) { // (the packet slots: ddn_fsk4_chain_set_m17_packet_slots may change their number until the first run)
        const size_t BP = (size_t)c->B * (size_t)c->m17.P;
        DDN_TRY(alloc_rc(BUF(m17.packet, BP * 832) && BUF(m17.packet_len, BP) && BUF(m17.packet_ok, BP) && BUF(m17.packet_slot, BP)));
    }
    DDN_TRY(ddn_m17_pkt_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_spat, c->d_ns, c->d_thr, c->B, (size_t)c->myd, c->m17.p26,
                                     c->m17.pf_st, c->m17.p_cost, st));
    DDN_TRY(ddn_m17_brt_decode_batch(rec, c->stride, c->d_cnt_full, c->d_spos, c->d_spat, c->d_ns, c->B, (size_t)c->myd, c->m17.b25,
                                     c->m17.bf_st, st));
    HIP_TRY(hipEventRecord(c->ev_reads, st)); // (the walk reads the sync lists too, but they are the decode stage's own copies)
    DDN_TRY(ddn_m17_data_assemble_batch(c->d_spat, c->d_spos, c->d_ns, c->d_new[cur], c->B, (size_t)c->myd, c->m17.p26, c->m17.pf_st,
                                        c->m17.b25, c->m17.bf_st, c->m17.data_state, c->m17.p_st, c->m17.p_cnt, c->m17.b_state,
                                        c->m17.packet, c->m17.packet_len, c->m17.packet_ok, c->m17.packet_slot, c->m17.n_packets, c->m17.P,
                                        st));
    return DDN_OK;
}

// ---- DMR ----------------------------------------------------------------------------------------------------------------------------
static int
dmr_alloc(ddn_fsk4_chain* c) {
    const size_t B = (size_t)c->B, S = c->S;
    DDN_TRY(alloc_rc(BUF(dmr.st, S * 20) && BUF(dmr.info, S * 196) && BUF(dmr.cach, S * 24) && BUF(dmr.valid, S) && BUF(dmr.st_ok, S)
                       && BUF(dmr.pdu, S * 96) && BUF(dmr.r3, S * 3) && BUF(dmr.errs, S)));
    if (!c->cfg.handlers) {
        return DDN_OK;
    }
    // the handlers' decisions of every call (events): which bursts go to dmr_data_burst_handler(), which to the vocoder,
    // under which VC a burst's sync field was filed.  Data bursts: at most one per 144 symbols; an embedded link control
    // per six voice bursts of a time slot
    c->dmr.E = (int)(c->ms / 36 + 32);
    c->dmr.db = (int)(c->ms / 144 + 3);
    c->dmr.lb = (int)(c->ms / (288 * 6) + 2);
    c->dmr.D = B * (size_t)c->dmr.db;
    c->dmr.L = 2 * B * (size_t)c->dmr.lb;
    const size_t D = c->dmr.D, L = c->dmr.L;
    DDN_TRY(alloc_rc(
        BUF(dmr.ev, B * (size_t)c->dmr.E * 4) && BUF(dmr.nev, B) && BUF(dmr.data.start, D) && BUF(dmr.data.pre, D) && BUF(dmr.data.n, B)
        && BUF(dmr.data.listn, D) && BUF(dmr.data.pooln, D) && BUF(dmr.emb.pos, L) && BUF(dmr.emb.n, 2 * B) && BUF(dmr.data.errs, D)
        && BUF(dmr.emb.errs, L) && BUF(dmr.data.slot, D) && BUF(dmr.data.st, D * 20) && BUF(dmr.data.st_ok, D) && BUF(dmr.data.info, D * 196)
        && BUF(dmr.data.td, D * 98) && BUF(dmr.data.rel, D * 98) && BUF(dmr.data.pdu, D * 96) && BUF(dmr.data.r3, D * 3) && BUF(dmr.data.type, D)
        && BUF(dmr.data.bytes, D * 12) && BUF(dmr.data.cw, D * 12) && BUF(dmr.data.rsres, D) && BUF(dmr.data.rsfound, D) && BUF(dmr.data.crc, D)
        && BUF(dmr.data.want, D) && BUF(dmr.data.hard, D * 18) && BUF(dmr.data.soft, D * 18) && BUF(dmr.data.list, D * 32 * 24)
        && BUF(dmr.data.backs, D * 49 * 8 * 32) && BUF(dmr.data.pool, D * 34 * 24) && BUF(dmr.data.unconf, D * 18) && BUF(dmr.data.conf, D * 18)
        && BUF(dmr.data.confcrc, D) && BUF(dmr.emb.sig, B * 2 * 7 * 48) && BUF(dmr.emb.in, L * 128) && BUF(dmr.emb.out, L * 77) && BUF(dmr.emb.ok, L)));
    DDN_TRY(ddn_fsk4_rx_set_events(c->rx, c->dmr.ev, c->dmr.nev, (size_t)c->dmr.E));
    if (!c->cfg.vocoder) {
        return DDN_OK;
    }
    // voice (dmrBSBootstrap / dmrBS -> processMbeFrame, dmr_bs.c:128-200,585-640): a time slot carries a burst every
    // 288 symbols, three AMBE 3600x2450 frames each; which bursts reach the vocoder is the handlers' decision (events)
    c->dmr.vb = (int)(c->ms / 288 + 3);
    c->V = 2 * B * (size_t)c->dmr.vb; // bursts
    const size_t V = c->V;
    DDN_TRY(alloc_rc(BUF(dmr.vstart, V) && BUF(dmr.vpre, V) && BUF(dmr.vnb, 2 * B) && BUF(d_ambe_fr, V * 3 * 96)));
    return voice_tail_alloc(c, V * 3, 2 * c->B);
}

// data PDUs (ddn_fsk4_chain_set_dmr_pdu_slots): where the events and the call's new flags put dmr_reset_blocks() and carrier loss
// among the bursts, then the walk over the data-burst stage's arrays; the state block starts all zeros (= a stream's start)
static void
dmr_pdu_output(const ddn_fsk4_chain* c, ddn_dmr_pdu_output* o) {
    const auto& p = c->dmr.pw;
    *o = ddn_dmr_pdu_output{p.P,   p.b_conf, p.b_counter, p.b_crc, p.b_dbsn, p.b_pick, p.b_status, p.n_pdus,
                            p.kind, p.slot,   p.burst,     p.len,   p.bytes,  p.crc4,   p.bcrc,     p.hdr};
}

static int
dmr_pdu_walk(ddn_fsk4_chain* c, int cur, hipStream_t st) {
    auto& p = c->dmr.pw;
    const size_t B = (size_t)c->B, D = c->dmr.D;
    if (!p.state) { // (the PDU slots: their number may change until the first run)
        const size_t BP = B * (size_t)p.P, BM = B * (size_t)p.M;
        DDN_TRY(alloc_rc(BUF(dmr.pw.state, B * ddn_dmr_pdu_state_bytes()) && BUF(dmr.pw.rb, BM) && BUF(dmr.pw.nr, B) && BUF(dmr.pw.lb, BM)
                           && BUF(dmr.pw.nl, B) && BUF(dmr.pw.b_conf, D) && BUF(dmr.pw.b_counter, D) && BUF(dmr.pw.b_crc, D)
                           && BUF(dmr.pw.b_dbsn, D) && BUF(dmr.pw.b_pick, D) && BUF(dmr.pw.b_status, D) && BUF(dmr.pw.n_pdus, B)
                           && BUF(dmr.pw.kind, BP) && BUF(dmr.pw.slot, BP) && BUF(dmr.pw.burst, BP) && BUF(dmr.pw.len, BP)
                           && BUF(dmr.pw.bytes, BP * 3072) && BUF(dmr.pw.crc4, BP * 4) && BUF(dmr.pw.bcrc, BP * 128) && BUF(dmr.pw.hdr, BP * 9)));
    }
    DDN_TRY(ddn_dmr_pdu_marks_batch(c->dmr.ev, c->dmr.nev, (size_t)c->dmr.E, c->d_fl[cur], c->stride, c->T, c->d_new[cur], c->dmr.data.start,
                                    c->dmr.data.n, c->B, c->dmr.db, p.state, p.rb, p.nr, p.lb, p.nl, p.M, st));
    ddn_dmr_pdu_input in{c->B,           c->dmr.db,        p.M,           c->dmr.data.n, c->dmr.data.slot, c->dmr.data.type, c->dmr.data.bytes,
                         c->dmr.data.info, c->dmr.data.errs, c->dmr.data.crc, c->dmr.data.unconf, c->dmr.data.pool, c->dmr.data.pooln,
                         p.nr,           p.rb,             p.nl,          p.lb};
    ddn_dmr_pdu_output out;
    dmr_pdu_output(c, &out);
    return ddn_dmr_pdu_walk_batch(&in, p.state, &out, st);
}

// MS / direct-mode bursts (ddn_fsk4_chain_set_dmr_ms): the buffers of the feature, made when it is enabled.  Syncs lie at least 288
// symbols apart behind a data word and 1728 behind a voice word, a unit's bursts 288: a call of ms new symbols ends ms / 288 + 2
// bursts of either kind at most and ms / 1728 + 2 units
static int
dmr_ms_alloc(ddn_fsk4_chain* c) {
    auto& p = c->dmr.ms;
    const size_t B = (size_t)c->B;
    p.b.max_data = p.b.max_voice = (int)(c->ms / 288 + 2);
    p.b.max_lc = (int)(c->ms / 1728 + 2);
    const size_t D = B * (size_t)p.b.max_data, V = B * (size_t)p.b.max_voice, L = B * (size_t)p.b.max_lc;
    uint8_t* pool = nullptr;
    DDN_TRY(alloc_rc(
        BUF(dmr.ms.state, B * ddn_dmr_ms_state_bytes()) && BUF(dmr.ms.b.d_n_data, B) && BUF(dmr.ms.b.d_data_start, D) && BUF(dmr.ms.b.d_data_sync, D)
        && BUF(dmr.ms.b.d_data_gate, D) && BUF(dmr.ms.b.d_data_pat, D) && BUF(dmr.ms.b.d_data_slot, D) && BUF(dmr.ms.b.d_data_status, D)
        && BUF(dmr.ms.b.d_data_cc, D) && BUF(dmr.ms.b.d_n_voice, B) && BUF(dmr.ms.b.d_voice_start, V) && BUF(dmr.ms.b.d_voice_pre, V)
        && BUF(dmr.ms.b.d_voice_vc, V) && BUF(dmr.ms.b.d_voice_tact_ok, V) && BUF(dmr.ms.b.d_voice_emb_ok, V) && BUF(dmr.ms.b.d_voice_emb_cc, V)
        && BUF(dmr.ms.b.d_voice_power, V) && BUF(dmr.ms.b.d_voice_sync48, V * 48) && BUF(dmr.ms.b.d_n_lc, B) && BUF(dmr.ms.b.d_lc_pos, L)
        && BUF(dmr.ms.b.d_lc_in128, L * 128) && BUF(dmr.ms.b.d_cc, B) && BUF(dmr.ms.b.d_dropped, B) && BUF(dmr.ms.b.d_phase, B)
        && BUF(dmr.ms.d.d_type, D) && BUF(dmr.ms.d.d_info196, D * 196) && BUF(dmr.ms.d.d_bits96, D * 96) && BUF(dmr.ms.d.d_bytes12, D * 12)
        && BUF(dmr.ms.d.d_errs, D) && BUF(dmr.ms.d.d_crc, D) && BUF(dmr.ms.d.d_r34_unconfirmed, D * 18) && BUF(dmr.ms.d.d_r34_confirmed, D * 18)
        && BUF(dmr.ms.d.d_r34_confirmed_crc, D) && c->pool.alloc(&pool, D * 34 * 24) && BUF(dmr.ms.d.d_r34_pool_n, D)
        && BUF(dmr.ms.v.d_ambe_frames, V * 3 * 96) && BUF(dmr.ms.v.d_skip, V * 3) && BUF(dmr.ms.v.d_lc77, L * 77) && BUF(dmr.ms.v.d_lc_errs, L)
        && BUF(dmr.ms.v.d_lc_ok, L)));
    p.d.d_r34_pool = pool;
    if (c->cfg.vocoder) {
        DDN_TRY(alloc_rc(BUF(dmr.ms.v.d_ambe_bits, V * 3 * 49) && BUF(dmr.ms.v.d_ambe_result, V * 3 * 5) && BUF(dmr.ms.v.d_pcm, V * 3 * 160)));
        DDN_TRY(ddn_mbe_batch_create(DDN_MBE_AMBE_3600X2450, c->B, &p.mbe));
    }
    DDN_TRY(ddn_dmr_ms_state_init(p.state, B, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return DDN_OK;
}

// (all of it ahead of ev_reads: the walk and both gathers read the records and the decode list's hand-overs)
static int
dmr_ms_stage(ddn_fsk4_chain* c, int cur, hipStream_t st) {
    const auto& p = c->dmr.ms;
    const ddn_dmr_ms_input in{c->B, c->stride, (size_t)c->myd, c->d_rec[cur], c->d_cnt_full, c->d_new[cur], c->d_spos, c->d_spat, c->d_ns, c->d_pre,
                              c->d_prel};
    DDN_TRY(ddn_dmr_ms_walk_batch(&in, p.state, &p.b, st));
    DDN_TRY(ddn_dmr_ms_data_batch(&in, &p.b, &p.d, st));
    return ddn_dmr_ms_voice_batch(&in, &p.b, &p.v, p.mbe, st);
}

static int
dmr_decode(ddn_fsk4_chain* c, int cur, int flush, hipStream_t st) {
    const size_t S = c->S;
    const uint8_t* rec = c->d_rec[cur];
    if (c->dmr.ms.on) {
        DDN_TRY(dmr_ms_stage(c, cur, st));
    }
    // burst gather -> slot type Golay(20,8) -> BPTC(196,96); an RC sync (pattern 8) carries no burst: its slot stays invalid
    HIP_TRY(ddn_dev_dmr_burst_gather(rec, c->d_cnt_full, c->stride, c->d_spos, c->d_spat, c->d_pre, c->d_ns, c->B, (int)c->myd,
                                     c->cfg.inverted, c->dmr.st, c->dmr.info, c->dmr.cach, c->dmr.valid, st));
    DDN_TRY(ddn_fec_block_code_batch(5 /* DDN_CODE_GOLAY_20_8 */, c->dmr.st, S, 1, nullptr, c->dmr.st_ok, st));
    DDN_TRY(ddn_fec_bptc_196x96_batch(c->dmr.info, 1, S, c->dmr.pdu, c->dmr.r3, c->dmr.errs, st));
    if (c->dmr.E && flush) { // no new records, no new decisions
        HIP_TRY(hipMemsetAsync(c->dmr.nev, 0, sizeof(int32_t) * (size_t)c->B, st));
    }
    if (c->dmr.E) {
        // the bursts the handlers dispatched to dmr_data_burst_handler() in this call (each ends inside it; one that began in the
        // previous call reaches back into the carried records): slot type, BPTC(196,96), the type's CRC / RS(12,9), and for
        // rate 3/4 bursts the three trellis decoders and the candidate pool (dmr_dburst.c:502-536)
        const size_t D = c->dmr.D, L = c->dmr.L;
        HIP_TRY(ddn_dev_dmr_data_select(c->dmr.ev, c->dmr.nev, c->dmr.E, c->T, c->B, c->dmr.db, c->d_spos, c->d_ns, c->myd, c->c_pos[cur], c->c_n[cur],
                                        c->myc, c->d_new[cur], c->dmr.data.start, c->dmr.data.slot, c->dmr.data.pre, c->dmr.data.n, st));
        HIP_TRY(ddn_dev_dmr_data_gather(rec, c->stride, c->dmr.data.start, c->dmr.data.pre, c->d_pre, c->d_prel, c->c_pre[cur], c->c_prel[cur],
                                        (long)c->S, c->dmr.db, c->B, c->dmr.data.st, c->dmr.data.info, c->dmr.data.td, c->dmr.data.rel, st));
        DDN_TRY(ddn_fec_block_code_batch(5 /* DDN_CODE_GOLAY_20_8 */, c->dmr.data.st, D, 1, nullptr, c->dmr.data.st_ok, st));
        DDN_TRY(ddn_fec_bptc_196x96_batch(c->dmr.data.info, 1, D, c->dmr.data.pdu, c->dmr.data.r3, c->dmr.data.errs, st));
        HIP_TRY(ddn_dev_dmr_data_prep(c->dmr.data.start, c->dmr.data.st, c->dmr.data.st_ok, c->dmr.data.pdu, (int)D, c->dmr.data.type, c->dmr.data.bytes, c->dmr.data.cw, st));
        DDN_TRY(ddn_fec_rs_12_9_batch(c->dmr.data.cw, D, c->dmr.data.rsres, c->dmr.data.rsfound, nullptr, st));
        HIP_TRY(ddn_dev_dmr_data_finish(c->dmr.data.type, c->dmr.data.pdu, c->dmr.data.info, c->dmr.data.cw, c->dmr.data.rsres, (int)D, c->dmr.data.bytes, c->dmr.data.crc,
                                        c->dmr.data.want, st));
        DDN_TRY(ddn_fec_r34_batch(c->dmr.data.td, nullptr, D, c->dmr.data.hard, st));
        DDN_TRY(ddn_fec_r34_batch(c->dmr.data.td, c->dmr.data.rel, D, c->dmr.data.soft, st));
        HIP_TRY(ddn_dev_r34_list_wanted(c->dmr.data.td, c->dmr.data.rel, (int)D, 32, c->dmr.data.want, c->dmr.data.backs, (uint32_t*)c->dmr.data.list, c->dmr.data.listn, st));
        HIP_TRY(ddn_dev_dmr_r34_pick(c->dmr.data.td, c->dmr.data.rel, c->dmr.data.want, c->dmr.data.hard, c->dmr.data.soft, c->dmr.data.list, c->dmr.data.listn, (int)D, c->dmr.data.pool,
                                     c->dmr.data.pooln, c->dmr.data.unconf, c->dmr.data.conf, c->dmr.data.confcrc, st));
        // embedded link control: the sync fields filed under VC 2..6, BPTC(128,77) at every voice burst with VC 6
        HIP_TRY(ddn_dev_dmr_emb_collect(c->dmr.ev, c->dmr.nev, c->dmr.E, c->T, rec, c->stride, c->B, c->dmr.lb, c->dmr.emb.sig, c->dmr.emb.in, c->dmr.emb.pos,
                                        c->dmr.emb.n, st));
        DDN_TRY(ddn_fec_bptc_128x77_batch(c->dmr.emb.in, L, c->dmr.emb.out, c->dmr.emb.errs, st));
        HIP_TRY(ddn_dev_dmr_emb_finish(c->dmr.emb.out, c->dmr.emb.pos, (int)L, c->dmr.emb.ok, st));
        if (c->dmr.pw.P) {
            DDN_TRY(dmr_pdu_walk(c, cur, st));
        }
    }
    if (!c->mbe) {
        HIP_TRY(hipEventRecord(c->ev_reads, st));
        return DDN_OK;
    }
    // voice: the bursts the handlers handed to the vocoder in this call (they end inside it; a burst that began in the
    // previous call reaches back into the carried records), filed by time slot -> 3 AMBE frames -> frame FEC -> synthesis.
    // (hard bits: the reference passes no soft frame here, processMbeFrame(opts, state, NULL, frame, NULL))
    const size_t V3 = c->V * 3;
    HIP_TRY(ddn_dev_dmr_voice_select(c->dmr.ev, c->dmr.nev, c->dmr.E, c->T, c->d_spos, c->d_ns, c->myd, c->B, c->dmr.vb, c->dmr.vstart,
                                     c->dmr.vpre, c->dmr.vnb, c->c_pos[cur], c->c_n[cur], c->myc, c->d_new[cur], st));
    HIP_TRY(ddn_dev_dmr_voice_gather_paths(rec, c->d_cnt_full, c->stride, c->dmr.vstart, c->dmr.vpre, c->d_pre, c->dmr.vb, c->B, 0,
                                           c->d_ambe_fr, c->d_skip, c->c_pre[cur], (long)c->S, st));
    HIP_TRY(hipEventRecord(c->ev_reads, st)); // (everything below works on the gathered frames)
    DDN_TRY(ddn_mbe_frame_decode_batch(DDN_MBE_AMBE_3600X2450, c->d_ambe_fr, nullptr, V3, c->d_ambe_d, c->d_ambe_res, st));
    DDN_TRY(ddn_mbe_result_skip_batch(c->d_skip, V3, c->d_ambe_res, st));
    DDN_TRY(ddn_mbe_synth_batch(c->mbe, c->d_ambe_d, c->d_ambe_res, (size_t)c->dmr.vb * 3, c->d_pcm, c->d_res_out, st));
    return DDN_OK;
}

// ---- NXDN48 / NXDN96 ----------------------------------------------------------------------------------------------------------------
static int
nxdn_alloc(ddn_fsk4_chain* c) {
    const size_t B = (size_t)c->B, S = c->S;
    // voice: four AMBE frames per NXDN frame, one talk path per channel.  With the handlers deciding the frame length two
    // syncs are at least a 192-symbol frame apart: a call decodes n / (192 * 20) + 3 frames at most
    const size_t cap = (size_t)c->n / (192 * 20) + 3;
    c->nxdn.vf = (int)(c->cfg.handlers ? (cap < (size_t)c->myd ? cap : (size_t)c->myd) : (size_t)c->myd);
    c->V = B * (size_t)c->nxdn.vf;
    const size_t V = c->V;
    DDN_TRY(alloc_rc(BUF(nxdn.lich, S) && BUF(nxdn.valid, S) && BUF(nxdn.ss, S * 72) && BUF(nxdn.sr, S * 72) && BUF(nxdn.fs, S * 384)
                       && BUF(nxdn.fr, S * 384) && BUF(nxdn.sacch, S * 4) && BUF(nxdn.sacch_ok, S) && BUF(nxdn.hard_in, S * 72)
                       && BUF(nxdn.sacch_hard, S * 32) && BUF(nxdn.sacch_hard_ok, S) && BUF(nxdn.facch, S * 2 * 12) && BUF(nxdn.facch_ok, S * 2)
                       && BUF(nxdn.vpos, V) && BUF(d_vn, B) && BUF(d_ambe_fr, V * 384) && BUF(d_ambe_rel, V * 384)));
    return voice_tail_alloc(c, V * 4, c->B);
}

// CAC / FACCH2 / UDCH frames and the SACCH walk (ddn_fsk4_chain_set_nxdn_ctrl): the buffers of the feature, made when it is
// enabled; the state block starts as ddn_nxdn_ctrl_state_init leaves it
static int
nxdn_ctrl_alloc(ddn_fsk4_chain* c) {
    const size_t B = (size_t)c->B, S = c->S;
    DDN_TRY(alloc_rc(BUF(nxdn.ctrl.state, B * ddn_nxdn_ctrl_state_bytes()) && BUF(nxdn.ctrl.kind, S) && BUF(nxdn.ctrl.bits, S * 208)
                       && BUF(nxdn.ctrl.bytes, S * 26) && BUF(nxdn.ctrl.crc, S) && BUF(nxdn.ctrl.fallback, S) && BUF(nxdn.ctrl.ran, S)
                       && BUF(nxdn.ctrl.sf, S) && BUF(nxdn.ctrl.sacch_status, S) && BUF(nxdn.ctrl.pf, S) && BUF(nxdn.ctrl.seq, S)
                       && BUF(nxdn.ctrl.msg, S * 72) && BUF(nxdn.ctrl.msg_status, S) && BUF(nxdn.ctrl.last_ran, S)
                       && BUF(nxdn.ctrl.cac_fail, S)));
    DDN_TRY(ddn_nxdn_ctrl_state_init(c->nxdn.ctrl.state, B, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return DDN_OK;
}

static void
nxdn_ctrl_outputs(const ddn_fsk4_chain* c, ddn_nxdn_ctrl_frames* fr, ddn_nxdn_ctrl_messages* ms) {
    const auto& p = c->nxdn.ctrl;
    *fr = ddn_nxdn_ctrl_frames{p.kind, p.bits, p.bytes, p.crc, p.fallback, p.ran, p.sf};
    *ms = ddn_nxdn_ctrl_messages{p.sacch_status, p.pf, p.seq, p.msg, p.msg_status, p.last_ran, p.cac_fail};
}

// (the records of this call's buffer set are written again by the loop of the call after the next, which waits for the whole of the
// next decode stage: the gather may read them behind ev_reads; the sync list and the counts are the decode stage's own copies)
static int
nxdn_ctrl_stage(ddn_fsk4_chain* c, int cur, hipStream_t st) {
    ddn_nxdn_ctrl_input in{c->B,           c->stride,          (size_t)c->myd,      c->d_rec[cur],        c->d_cnt_full, c->d_spos, c->d_ns, c->nxdn.lich,
                           c->nxdn.valid, c->nxdn.sacch, c->nxdn.sacch_ok, c->nxdn.sacch_hard, c->nxdn.sacch_hard_ok};
    ddn_nxdn_ctrl_frames fr;
    ddn_nxdn_ctrl_messages ms;
    nxdn_ctrl_outputs(c, &fr, &ms);
    DDN_TRY(ddn_nxdn_ctrl_decode_batch(&in, &fr, st));
    return ddn_nxdn_ctrl_walk_batch(&in, &fr, c->nxdn.ctrl.state, &ms, st);
}

// frame gather -> SACCH / FACCH1 K=5 soft decode -> CRC6 / CRC12 -> the reference's greedy retry for the SACCH
static int
nxdn_decode(ddn_fsk4_chain* c, int cur, int, hipStream_t st) {
    const size_t S = c->S;
    const uint8_t* rec = c->d_rec[cur];
    DDN_TRY(ddn_nxdn_frame_gather(rec, c->d_cnt_full, c->stride, c->d_spos, c->d_ns, c->B, (size_t)c->myd, c->nxdn.lich, c->nxdn.ss, c->nxdn.sr,
                                  c->nxdn.fs, c->nxdn.fr, c->nxdn.valid, st));
    if (c->cfg.vocoder) {
        // voice, first half: which frames the LICHs announce, and their AMBE words out of the records (both only need the frame
        // gather's LICHs; done here so that every reader of the loop's buffers sits at the head of the stage)
        HIP_TRY(ddn_dev_nxdn_voice_select(c->d_spos, c->d_ns, c->nxdn.lich, c->nxdn.valid, c->B, c->myd, c->nxdn.vf, c->nxdn.vpos, c->d_vn, c->d_skip, st));
        DDN_TRY(ddn_nxdn_voice_gather(rec, c->d_cnt_full, c->stride, c->nxdn.vpos, c->d_vn, c->B, (size_t)c->nxdn.vf, c->d_ambe_fr, c->d_ambe_rel,
                                      nullptr, st));
    }
    HIP_TRY(hipEventRecord(c->ev_reads, st)); // (the decoders and the synthesis below work on the gathered words)
    // (the decoders skip the slots that hold no complete frame - nxdn.valid - and write zeros there: the slot arrays are sized for the
    // densest traffic, a call of the bench capture uses an eighth of them)
    HIP_TRY(ddn_dev_k5_nxdn_wanted(c->nxdn.ss, c->nxdn.sr, (int)S, 36, 32, nullptr, c->nxdn.sacch, 4, c->nxdn.valid, 1, st));
    DDN_TRY(ddn_nxdn_crc_check_batch(c->nxdn.sacch, 4, S, 0, c->nxdn.sacch_ok, st));
    HIP_TRY(ddn_dev_u8_shr1(c->nxdn.ss, S * 72, c->nxdn.hard_in, st));
    HIP_TRY(ddn_dev_trellis_greedy_wanted(c->nxdn.hard_in, 72, S, 32, c->nxdn.sacch_hard, 32, c->nxdn.valid, st));
    DDN_TRY(ddn_nxdn_crc_check_batch(c->nxdn.sacch_hard, 32, S, 2, c->nxdn.sacch_hard_ok, st));
    HIP_TRY(ddn_dev_k5_nxdn_wanted(c->nxdn.fs, c->nxdn.fr, (int)(S * 2), 96, 92, nullptr, c->nxdn.facch, 12, c->nxdn.valid, 2, st));
    DDN_TRY(ddn_nxdn_crc_check_batch(c->nxdn.facch, 12, S * 2, 1, c->nxdn.facch_ok, st));
    if (c->cfg.vocoder) {
        // voice (nxdn_voice()): the frames the LICHs announce (selected and gathered above), through frame FEC -> synthesis
        const size_t V4 = c->V * 4;
        DDN_TRY(ddn_mbe_frame_decode_batch(DDN_MBE_AMBE_3600X2450, c->d_ambe_fr, c->d_ambe_rel, V4, c->d_ambe_d, c->d_ambe_res, st));
        DDN_TRY(ddn_mbe_result_skip_batch(c->d_skip, V4, c->d_ambe_res, st));
        DDN_TRY(ddn_mbe_synth_batch(c->mbe, c->d_ambe_d, c->d_ambe_res, (size_t)c->nxdn.vf * 4, c->d_pcm, c->d_res_out, st));
    }
    if (c->nxdn.ctrl.on) {
        DDN_TRY(nxdn_ctrl_stage(c, cur, st));
    }
    return DDN_OK;
}
#undef BUF

// One row per protocol, indexed by DDN_FSK4_* - the chain's own facts; the loop's (symbol rate, handler family) are in
// ddn_fsk4::kRow.  T: a DMR burst ends 54 symbols after its sync, an NXDN frame 182, an M17 frame 184;
// myc = 16 syncs can lie inside such a tail (a new sync needs 24 / 10 fresh symbols).
static const ddn_fsk4_traits fsk4_traits[] = {
    {},
    /* DMR    */ {4, DDN_LPF_12K5, 256, 0, false, -1, true, true, dmr_alloc, dmr_decode},
    /* NXDN48 */ {4, DDN_LPF_6K25, 256, 0, false, -1, true, true, nxdn_alloc, nxdn_decode},
    // (NXDN96: a 12.5 kHz channel at 4800 symbols/s)
    /* NXDN96 */ {4, DDN_LPF_12K5, 256, 0, false, -1, true, true, nxdn_alloc, nxdn_decode},
    /* M17    */ {4, DDN_LPF_12K5, 256, 0, true, 0, true, true, m17_alloc, m17_decode},
    // (a YSF frame's payload ends 460 symbols after its sync; the FICH ends 100 symbols after it)
    /* YSF    */ {4, DDN_LPF_12K5, 480, 0, false, 0, true, true, ysf_alloc, ysf_decode},
    // (a dPMR superframe ends 372 symbols after its sync.)  The loop holds 372 symbols behind every sync and then hunts a fresh
    // 12-symbol window, so accepted syncs lie at least 384 symbols apart and the ones a call decodes (positions below its new-record
    // count) number ms / 384 + 1 at most
    /* DPMR   */ {4, DDN_LPF_6K25, 480, 384, false, 1, true, false, dpmr_alloc, dpmr_decode},
    // (D-STAR: 4800 symbols/s behind the 6.25 kHz filter the reference picks for -fd, as ddn_host_mode.c does; a header unit ends
    // 660 + 1992 = 2652 symbols after its sync.)  1992 / 2652 symbols behind every sync, then a fresh 24-symbol window: syncs at least
    // 2016 symbols apart
    /* DSTAR  */ {4, DDN_LPF_6K25, 2688, 2016, true, 0, false, false, dstar_alloc, dstar_decode},
    // (EDACS: 9600 symbols/s, two levels, behind the ProVoice channel profile dsd_rtl_channel_profile_for(9600, 2, ..) picks,
    // src/runtime/decode_mode.c:83-99; a frame ends 240 symbols after its 48-symbol sync.)  240 symbols behind every sync, then a
    // fresh 48-symbol window: syncs at least 288 symbols apart
    /* EDACS  */ {2, DDN_LPF_PROVOICE, 320, 288, true, 0, false, false, edacs_alloc, edacs_decode},
};

extern "C" void
ddn_fsk4_chain_destroy(ddn_fsk4_chain* c) {
    if (!c) {
        return;
    }
    (void)hipDeviceSynchronize();
    if (c->ev_reads) {
        (void)hipEventDestroy(c->ev_reads);
    }
    ddn_batch_destroy(c->fe);
    ddn_fsk4_rx_destroy(c->rx);
    ddn_mbe_batch_destroy(c->mbe);
    ddn_mbe_batch_destroy(c->ysf.mbe_i);
    ddn_mbe_batch_destroy(c->dmr.ms.mbe);
    c->pool.release();
    delete c;
}

// everything create makes after the object itself; what a failure leaves behind is destroy's
static int
fsk4_setup(ddn_fsk4_chain* c) {
    const ddn_fsk4_chain_config* cfg = &c->cfg;
    const ddn_fsk4_traits* tr = c->tr;
    ddn_front_end_config fc = {c->B, 48000, ddn_fsk4::kRow[cfg->protocol].sym_rate, tr->levels, tr->lpf, cfg->input_format, cfg->block_len, 0.0f};
    DDN_TRY(ddn_batch_create(&fc, &c->fe));
    if (hipEventCreateWithFlags(&c->ev_reads, hipEventDisableTiming) != hipSuccess) {
        return DDN_EHIP;
    }
    ddn_fsk4_rx_config rcfg;
    memset(&rcfg, 0, sizeof(rcfg));
    rcfg.n_channels = c->B;
    rcfg.out_rate_hz = 48000;
    rcfg.protocol = cfg->protocol;
    rcfg.rf_mod = cfg->rf_mod;
    rcfg.inverted = cfg->inverted;
    rcfg.use_matched_filter = 1;
    DDN_TRY(ddn_fsk4_rx_create(&rcfg, &c->rx));
    if (cfg->handlers) {
        DDN_TRY(ddn_fsk4_rx_set_handlers(c->rx, 1));
    }
    c->ms = ddn_fsk4_rx_max_symbols(c->rx, (size_t)c->n);
    c->my = ddn_fsk4_rx_max_syncs(c->rx, (size_t)c->n);
    c->stride = (size_t)c->T + c->ms;
    // Decode slots per channel and call.  The loop's own bound (a sync per window length) is what noise could do in theory;
    // with the handlers in the loop accepted syncs are bursts / frames (144 / 192 symbols apart), so twice the densest real
    // traffic + the carried ones is what every decode launch is sized for - a sync beyond that is counted in d_dropped_syncs.
    // A protocol whose loop keeps accepted syncs min_sync_gap apart decodes ms / min_sync_gap + 1 of them per call at most.
    const size_t dense = c->ms / 64 + 24 + (size_t)c->myc, loop_bound = c->my + (size_t)c->myc;
    c->myd = (int)(cfg->handlers && dense < loop_bound ? dense : loop_bound);
    if (tr->min_sync_gap && c->ms / (size_t)tr->min_sync_gap + 4 < (size_t)c->myd) {
        c->myd = (int)(c->ms / (size_t)tr->min_sync_gap + 4);
    }
    c->S = (size_t)c->B * (size_t)c->myd;
    const size_t B = (size_t)c->B, S = c->S, my = c->my, myc = (size_t)c->myc;
    DdnPool& m = c->pool;
    bool ok = m.alloc(&c->d_disc, B * (size_t)c->n) && m.alloc(&c->d_pay, B * c->stride * 2) && m.alloc(&c->d_cnt_full, B)
              && m.alloc(&c->d_cnt_scan, B) && m.alloc(&c->d_dropped, B) && m.alloc(&c->s_pos, B * my) && m.alloc(&c->s_n, B)
              && m.alloc(&c->s_pat, B * my) && m.alloc(&c->s_pre, B * my * 90) && m.alloc(&c->s_prel, B * my * 90) && m.alloc(&c->d_spos, S)
              && m.alloc(&c->d_ns, B) && m.alloc(&c->d_spat, S) && m.alloc(&c->d_pre, S * 90) && m.alloc(&c->d_prel, S * 90);
    for (int k = 0; k < 2 && ok; k++) {
        ok = m.alloc(&c->d_rec[k], B * c->stride * 10) && m.alloc(&c->d_fl[k], B * c->stride) && m.alloc(&c->d_new[k], B)
             && m.alloc(&c->c_pos[k], B * myc) && m.alloc(&c->c_n[k], B) && m.alloc(&c->c_pat[k], B * myc)
             && m.alloc(&c->c_pre[k], B * myc * 90) && m.alloc(&c->c_prel[k], B * myc * 90);
    }
    DDN_TRY(alloc_rc(ok));
    if (tr->thresholds) {
        DDN_TRY(alloc_rc(m.alloc(&c->s_thr, B * my * 5) && m.alloc(&c->c_thr[0], B * myc * 5) && m.alloc(&c->c_thr[1], B * myc * 5)
                           && m.alloc(&c->d_thr, S * 5)));
        DDN_TRY(ddn_fsk4_rx_set_sync_thresholds(c->rx, c->s_thr));
    }
    return tr->alloc(c);
}

extern "C" int
ddn_fsk4_chain_create(const ddn_fsk4_chain_config* cfg, ddn_fsk4_chain** out) {
    static_assert(sizeof(fsk4_traits) / sizeof(fsk4_traits[0]) == ddn_fsk4::N_PROTO + 1, "one row per protocol of the loop");
    const ddn_fsk4_traits* tr = (cfg && ddn_fsk4::known(cfg->protocol)) ? &fsk4_traits[cfg->protocol] : nullptr;
    if (!tr || !out || cfg->n_channels <= 0 || cfg->samples_per_call <= 0 || cfg->block_len <= 0 || (cfg->handlers && !ddn_fsk4::kRow[cfg->protocol].handlers)
        || (tr->inverted_max >= 0 && (cfg->inverted < 0 || cfg->inverted > tr->inverted_max)) || (cfg->vocoder && !tr->vocoder)
        || (!tr->any_rf_mod && cfg->rf_mod != 0 && cfg->rf_mod != 2)) {
        ddn_set_error("ddn_fsk4_chain_create: bad configuration");
        return DDN_EINVAL;
    }
    if (ddn_input_format_bytes(cfg->input_format) == 0) {
        ddn_set_error("ddn_fsk4_chain_create: unknown input_format %d", cfg->input_format);
        return DDN_EINVAL;
    }
    *out = nullptr;
    ddn_fsk4_chain* c = new (std::nothrow) ddn_fsk4_chain();
    if (!c) {
        return DDN_ENOMEM;
    }
    c->cfg = *cfg;
    c->tr = tr;
    c->B = cfg->n_channels;
    c->n = cfg->samples_per_call;
    c->T = tr->T;
    c->myc = 16;
    c->m17.P = 4;
    const int rc = fsk4_setup(c);
    if (rc != DDN_OK) {
        ddn_fsk4_chain_destroy(c);
        return rc;
    }
    *out = c;
    return DDN_OK;
}

// frame FEC (+ voice) of the syncs this call decodes, out of buffer set `cur`
static int
fsk4_decode(ddn_fsk4_chain* c, int cur, int flush, hipStream_t st) {
    const int prev = cur ^ 1;
    HIP_TRY(ddn_dev_chain_counts(c->d_new[cur], c->T, c->B, flush, c->d_cnt_scan, c->d_cnt_full, st));
    HIP_TRY(ddn_dev_fsk4_chain_syncs_thr(c->c_pos[prev], c->c_pat[prev], c->c_pre[prev], c->c_prel[prev], c->c_n[prev], c->myc, c->s_pos,
                                         c->s_pat, c->s_pre, c->s_prel, c->s_n, (int)c->my, c->d_new[cur], c->T, flush, c->d_spos, c->d_spat,
                                         c->d_pre, c->d_prel, c->d_ns, c->myd, c->c_pos[cur], c->c_pat[cur], c->c_pre[cur], c->c_prel[cur],
                                         c->c_n[cur], c->d_dropped, c->B, c->s_thr ? c->c_thr[prev] : nullptr, c->s_thr, c->d_thr,
                                         c->s_thr ? c->c_thr[cur] : nullptr, st));
    return c->tr->decode(c, cur, flush, st);
}

// stage 0: front end, 1: carry + matched filter + receive loop, 2: frame FEC (+ voice)
extern "C" int
ddn_fsk4_chain_stage(ddn_fsk4_chain* c, int stage, const void* d_iq, void* hip_stream) {
    if (!c || stage < 0 || stage > 2 || (stage == 0 && !d_iq)) {
        return DDN_EINVAL;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int cur = (int)(c->step & 1), prev = cur ^ 1;
    float* disc = (c->d_disc2 && (c->step & 1)) ? c->d_disc2 : c->d_disc;
    if (stage == 0) {
        return ddn_front_end_run(c->fe, d_iq, (size_t)c->n, disc, st);
    }
    if (stage == 1) {
        HIP_TRY(ddn_dev_chain_carry(c->d_rec[prev], c->d_fl[prev], c->d_new[prev], c->step > 0 ? 1 : 0, c->d_rec[cur], c->d_fl[cur],
                                    c->stride, c->T, c->B, st));
        // the loop writes behind the T carried records: row pointers + T, row stride unchanged
        return ddn_fsk4_rx_run(c->rx, disc, (size_t)c->n, c->d_rec[cur] + (size_t)c->T * 10, c->d_fl[cur] + c->T,
                               c->d_pay + (size_t)c->T * 2, c->d_new[cur], c->stride, c->s_pos, c->s_pat, c->s_pre, c->s_prel, c->s_n,
                               c->my, st);
    }
    DDN_TRY(fsk4_decode(c, cur, 0, st));
    c->last_set = cur;
    c->step++;
    return DDN_OK;
}

// (internal, the mixed chain) the event the decode stage records once everything that reads the loop's buffers has been queued
extern "C" void*
ddn_fsk4_chain_reads_done_event(ddn_fsk4_chain* c) {
    return c ? (void*)c->ev_reads : nullptr;
}

// (internal, the mixed chain's shared front end) where this call's stage 0 would write its discriminator rows
extern "C" float*
ddn_fsk4_chain_disc_buffer(ddn_fsk4_chain* c) {
    return !c ? nullptr : ((c->d_disc2 && (c->step & 1)) ? c->d_disc2 : c->d_disc);
}

extern "C" int
ddn_fsk4_chain_run(ddn_fsk4_chain* c, const void* d_iq, void* hip_stream) {
    if (!c || !d_iq) {
        return DDN_EINVAL;
    }
    for (int stage = 0; stage < 3; stage++) {
        DDN_TRY(ddn_fsk4_chain_stage(c, stage, d_iq, hip_stream));
    }
    return DDN_OK;
}

// decode what the carry still holds back (end of a stream): one more decode pass without new samples
extern "C" int
ddn_fsk4_chain_flush(ddn_fsk4_chain* c, void* hip_stream) {
    if (!c) {
        return DDN_EINVAL;
    }
    if (c->step == 0) {
        return DDN_OK;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int cur = (int)(c->step & 1), prev = cur ^ 1;
    HIP_TRY(ddn_dev_chain_carry(c->d_rec[prev], c->d_fl[prev], c->d_new[prev], 1, c->d_rec[cur], c->d_fl[cur], c->stride, c->T, c->B, st));
    HIP_TRY(hipMemsetAsync(c->d_new[cur], 0, sizeof(int32_t) * (size_t)c->B, st));
    HIP_TRY(hipMemsetAsync(c->s_n, 0, sizeof(int32_t) * (size_t)c->B, st));
    DDN_TRY(fsk4_decode(c, cur, 1, st));
    c->last_set = cur;
    c->step++;
    HIP_TRY(hipStreamSynchronize(st));
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_results(ddn_fsk4_chain* c, ddn_fsk4_chain_results* r) {
    if (!c || !r) {
        return DDN_EINVAL;
    }
    const int cur = c->last_set, proto = c->cfg.protocol;
    memset(r, 0, sizeof(*r));
    r->stride_symbols = c->stride;
    r->carry_symbols = (size_t)c->T;
    r->max_syncs = (size_t)c->myd;
    r->voice_slots = c->nxdn.vf;
    r->d_records10 = c->d_rec[cur];
    r->d_flags = c->d_fl[cur];
    r->d_payload2 = c->d_pay;
    r->d_new = c->d_new[cur];
    r->d_counts = c->d_cnt_full;
    r->d_n_sync = c->d_ns;
    r->d_dropped_syncs = c->d_dropped;
    r->d_sync_pos = c->d_spos;
    r->d_sync_pat = c->d_spat;
    r->d_pre = c->d_pre;
    r->d_valid = proto == DDN_FSK4_DMR ? c->dmr.valid : c->nxdn.valid;
    r->d_dmr_slot_type = c->dmr.st;
    r->d_dmr_slot_type_ok = c->dmr.st_ok;
    r->d_dmr_pdu96 = c->dmr.pdu;
    r->d_dmr_bptc_errs = c->dmr.errs;
    r->d_nxdn_lich = c->nxdn.lich;
    r->d_nxdn_sacch = c->nxdn.sacch;
    r->d_nxdn_sacch_ok = c->nxdn.sacch_ok;
    r->d_nxdn_sacch_hard = c->nxdn.sacch_hard;
    r->d_nxdn_sacch_hard_ok = c->nxdn.sacch_hard_ok;
    r->d_nxdn_facch = c->nxdn.facch;
    r->d_nxdn_facch_ok = c->nxdn.facch_ok;
    if (proto == DDN_FSK4_DMR && c->dmr.E) {
        r->d_events = c->dmr.ev;
        r->d_n_events = c->dmr.nev;
        r->max_events = c->dmr.E;
        r->dmr_data_bursts = c->dmr.db;
        r->d_dmr_n_data = c->dmr.data.n;
        r->d_dmr_data_start = c->dmr.data.start;
        r->d_dmr_data_slot = c->dmr.data.slot;
        r->d_dmr_data_type = c->dmr.data.type;
        r->d_dmr_data_info196 = c->dmr.data.info;
        r->d_dmr_data_bits96 = c->dmr.data.pdu;
        r->d_dmr_data_bytes12 = c->dmr.data.bytes;
        r->d_dmr_data_errs = c->dmr.data.errs;
        r->d_dmr_data_crc = c->dmr.data.crc;
        r->d_dmr_r34_unconfirmed = c->dmr.data.unconf;
        r->d_dmr_r34_confirmed = c->dmr.data.conf;
        r->d_dmr_r34_confirmed_crc = c->dmr.data.confcrc;
        r->d_dmr_r34_pool = (const ddn_r34_candidate*)c->dmr.data.pool;
        r->d_dmr_r34_pool_n = c->dmr.data.pooln;
        r->dmr_emb_lcs = c->dmr.lb;
        r->d_dmr_n_emb = c->dmr.emb.n;
        r->d_dmr_emb_pos = c->dmr.emb.pos;
        r->d_dmr_emb_lc77 = c->dmr.emb.out;
        r->d_dmr_emb_errs = c->dmr.emb.errs;
        r->d_dmr_emb_ok = c->dmr.emb.ok;
    }
    if (proto == DDN_FSK4_DMR) {
        r->dmr_voice_bursts = c->dmr.vb;
        r->d_dmr_voice_start = c->dmr.vstart;
        r->d_dmr_voice_pre = c->dmr.vpre;
        r->d_dmr_n_voice = c->dmr.vnb;
        r->d_dmr_voice_skip = c->d_skip;
        r->d_dmr_ambe_frames = c->d_ambe_fr;
        r->d_dmr_ambe_bits = c->d_ambe_d;
        r->d_dmr_ambe_result = c->d_res_out;
        r->d_dmr_pcm = c->d_pcm;
        r->d_events = c->dmr.ev;
        r->d_n_events = c->dmr.nev;
        r->max_events = c->dmr.E;
    } else if (proto != DDN_FSK4_DPMR) {
        r->d_nxdn_voice_skip = c->d_skip;
        r->d_nxdn_ambe_bits = c->d_ambe_d;
        r->d_nxdn_pcm = c->d_pcm;
    }
    if (proto == DDN_FSK4_YSF) {
        r->d_ysf_fich4 = c->ysf.fich4;
        r->d_ysf_fich_status = c->ysf.st;
        r->d_ysf_fich_cost = c->ysf.ve;
        r->d_ysf_info2 = c->ysf.info;
        r->d_ysf_dch40 = c->ysf.dch;
        r->d_ysf_dch_status2 = c->ysf.dst;
        r->d_ysf_dch_cost2 = c->ysf.dcost;
        r->d_ysf_ambe49x5 = c->ysf.ambe;
        r->d_ysf_errs2x5 = c->ysf.errs;
        r->d_ysf_frames184x5 = c->ysf.fr;
        r->d_ysf_n_frames = c->ysf.nfr;
        r->ysf_voice_frames = c->mbe ? c->ysf.vf : 0;
        r->d_ysf_n_voice = c->mbe ? c->d_vn : nullptr;
        r->d_ysf_voice_slot = c->mbe ? c->ysf.vslot : nullptr;
        r->d_ysf_voice_result = c->mbe ? c->d_res_out : nullptr;
        r->d_ysf_pcm = c->mbe ? c->d_pcm : nullptr;
        r->d_ysf_voice_skip = c->mbe ? c->d_skip : nullptr;
        r->d_ysf_imbe_n_voice = c->ysf.mbe_i ? c->ysf.i_vn : nullptr;
        r->d_ysf_imbe_voice_slot = c->ysf.mbe_i ? c->ysf.i_vslot : nullptr;
        r->d_ysf_imbe_voice_skip = c->ysf.mbe_i ? c->ysf.i_skip : nullptr;
        r->d_ysf_imbe_voice_result = c->ysf.mbe_i ? c->ysf.i_res_out : nullptr;
        r->d_ysf_imbe_pcm = c->ysf.mbe_i ? c->ysf.i_pcm : nullptr;
    }
    if (proto == DDN_FSK4_M17) {
        r->d_sync_thr5 = c->d_thr;
        r->d_m17_lsf30 = c->m17.lsf;
        r->d_m17_lsf_status = c->m17.lsf_st;
        r->d_m17_lsf_cost = c->m17.cost;
        r->d_m17_lich6 = c->m17.l6;
        r->d_m17_lich_cnt = c->m17.cnt;
        r->d_m17_fn_payload18 = c->m17.fp;
        r->d_m17_str_status = c->m17.st;
        r->d_m17_lich_lsf30 = c->m17.ll;
        r->d_m17_lich_status = c->m17.ll_st;
    }
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_dpmr_results(ddn_fsk4_chain* c, ddn_dpmr_chain_results* r) {
    if (!c || !r || c->cfg.protocol != DDN_FSK4_DPMR) {
        ddn_set_error("ddn_fsk4_chain_get_dpmr_results: not a dPMR chain");
        return DDN_EINVAL;
    }
    memset(r, 0, sizeof(*r));
    r->max_syncs = (size_t)c->myd;
    r->voice_frames = c->mbe ? c->dpmr.vf : 0;
    r->d_n_sync = c->d_ns;
    r->d_sync_pos = c->d_spos;
    r->d_valid = c->dpmr.valid;
    r->d_cch_bits2x48 = c->dpmr.bits;
    r->d_ham_ok2x6 = c->dpmr.ham;
    r->d_crc_ok2 = c->dpmr.crc;
    r->d_fields2x8 = c->dpmr.fields;
    r->d_id = c->dpmr.id;
    r->d_color = c->dpmr.color;
    r->d_kind = c->dpmr.kind;
    r->d_strong = c->dpmr.strong;
    r->d_tg = c->dpmr.tg;
    r->d_src = c->dpmr.src;
    if (c->mbe) {
        r->d_ambe_fr = c->dpmr.fr;
        r->d_voiced2 = c->dpmr.voiced;
        r->d_muted2 = c->dpmr.muted;
        r->d_n_voice = c->d_vn;
        r->d_voice_slot = c->dpmr.vslot;
        r->d_voice_half = c->dpmr.vhalf;
        r->d_voice_muted = c->dpmr.vmuted;
        r->d_voice_skip = c->d_skip;
        r->d_voice_result = c->d_res_out;
        r->d_pcm = c->d_pcm;
    }
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_dstar_results(ddn_fsk4_chain* c, ddn_dstar_chain_results* r) {
    if (!c || !r || c->cfg.protocol != DDN_FSK4_DSTAR) {
        ddn_set_error("ddn_fsk4_chain_get_dstar_results: not a D-STAR chain");
        return DDN_EINVAL;
    }
    memset(r, 0, sizeof(*r));
    r->max_syncs = (size_t)c->myd;
    r->d_n_sync = c->d_ns;
    r->d_sync_pos = c->d_spos;
    r->d_sync_pat = c->d_spat;
    r->d_sync_thr5 = c->d_thr;
    r->d_hdr41 = c->dstar.h41;
    r->d_hdr_crc_ok = c->dstar.hok;
    r->d_hdr_valid = c->dstar.hv;
    r->d_ambe_fr = c->dstar.ambe;
    r->d_sd_bytes = c->dstar.sdb;
    r->d_sd_kind = c->dstar.kind;
    r->d_sd_hdr41 = c->dstar.sh41;
    r->d_sd_crc_ok = c->dstar.sok;
    r->d_sd_text = c->dstar.text;
    r->d_valid = c->dstar.vv;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_set_m17_packet_slots(ddn_fsk4_chain* c, int max_packets) {
    if (!c || c->cfg.protocol != DDN_FSK4_M17 || c->step != 0 || max_packets < 1 || max_packets > 33) {
        ddn_set_error("ddn_fsk4_chain_set_m17_packet_slots: an M17 chain before its first run, 1 .. 33 packet slots");
        return DDN_EINVAL;
    }
    c->m17.P = max_packets;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_m17_data_results(ddn_fsk4_chain* c, ddn_m17_data_chain_results* r) {
    if (!c || !r || c->cfg.protocol != DDN_FSK4_M17) {
        ddn_set_error("ddn_fsk4_chain_get_m17_data_results: not an M17 chain");
        return DDN_EINVAL;
    }
    memset(r, 0, sizeof(*r));
    r->max_syncs = (size_t)c->myd;
    r->max_packets = c->m17.P;
    r->d_n_sync = c->d_ns;
    r->d_sync_pos = c->d_spos;
    r->d_sync_pat = c->d_spat;
    r->d_pkt26 = c->m17.p26;
    r->d_pkt_frame_status = c->m17.pf_st;
    r->d_pkt_cost = c->m17.p_cost;
    r->d_bits25 = c->m17.b25;
    r->d_brt_frame_status = c->m17.bf_st;
    r->d_pkt_status = c->m17.p_st;
    r->d_pkt_count = c->m17.p_cnt;
    r->d_brt_state = c->m17.b_state;
    r->d_n_packets = c->m17.n_packets;
    r->d_packet = c->m17.packet;
    r->d_packet_app_len = c->m17.packet_len;
    r->d_packet_crc_ok = c->m17.packet_ok;
    r->d_packet_slot = c->m17.packet_slot;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_set_dmr_pdu_slots(ddn_fsk4_chain* c, int max_pdus) {
    if (!c || c->cfg.protocol != DDN_FSK4_DMR || !c->cfg.handlers || c->step != 0 || max_pdus < 1 || max_pdus > 8) {
        ddn_set_error("ddn_fsk4_chain_set_dmr_pdu_slots: a DMR chain with handlers = 1 before its first run, 1 .. 8 PDU slots");
        return DDN_EINVAL;
    }
    c->dmr.pw.P = max_pdus;
    c->dmr.pw.M = c->dmr.E; // (a mark needs an event or 1800 symbols)
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_dmr_pdu_results(ddn_fsk4_chain* c, ddn_dmr_pdu_chain_results* r) {
    if (!c || !r || c->cfg.protocol != DDN_FSK4_DMR || !c->dmr.pw.P) {
        ddn_set_error("ddn_fsk4_chain_get_dmr_pdu_results: a DMR chain with ddn_fsk4_chain_set_dmr_pdu_slots called");
        return DDN_EINVAL;
    }
    memset(r, 0, sizeof(*r));
    r->dmr_data_bursts = c->dmr.db;
    r->max_marks = c->dmr.pw.M;
    r->d_n_resets = c->dmr.pw.nr;
    r->d_reset_before = c->dmr.pw.rb;
    r->d_n_losses = c->dmr.pw.nl;
    r->d_loss_before = c->dmr.pw.lb;
    dmr_pdu_output(c, &r->out);
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_set_nxdn_ctrl(ddn_fsk4_chain* c, int enable) {
    if (!c || (c->cfg.protocol != DDN_FSK4_NXDN48 && c->cfg.protocol != DDN_FSK4_NXDN96) || !c->cfg.handlers || c->step != 0
        || (enable != 0 && enable != 1)) {
        ddn_set_error("ddn_fsk4_chain_set_nxdn_ctrl: an NXDN48 / NXDN96 chain with handlers = 1 before its first run, enable 0 / 1");
        return DDN_EINVAL;
    }
    if (enable && !c->nxdn.ctrl.state) {
        DDN_TRY(nxdn_ctrl_alloc(c));
    }
    c->nxdn.ctrl.on = enable;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_nxdn_ctrl_results(ddn_fsk4_chain* c, ddn_nxdn_ctrl_chain_results* r) {
    if (!c || !r || (c->cfg.protocol != DDN_FSK4_NXDN48 && c->cfg.protocol != DDN_FSK4_NXDN96) || !c->nxdn.ctrl.on) {
        ddn_set_error("ddn_fsk4_chain_get_nxdn_ctrl_results: an NXDN48 / NXDN96 chain with ddn_fsk4_chain_set_nxdn_ctrl enabled");
        return DDN_EINVAL;
    }
    memset(r, 0, sizeof(*r));
    r->max_syncs = (size_t)c->myd;
    r->d_n_sync = c->d_ns;
    r->d_sync_pos = c->d_spos;
    r->d_valid = c->nxdn.valid;
    nxdn_ctrl_outputs(c, &r->frames, &r->messages);
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_set_dmr_ms(ddn_fsk4_chain* c, int enable) {
    if (!c || c->cfg.protocol != DDN_FSK4_DMR || !c->cfg.handlers || c->cfg.inverted != 0 || c->step != 0 || (enable != 0 && enable != 1)) {
        ddn_set_error("ddn_fsk4_chain_set_dmr_ms: a DMR chain with handlers = 1 and inverted = 0 before its first run, enable 0 / 1");
        return DDN_EINVAL;
    }
    if (enable && !c->dmr.ms.state) {
        DDN_TRY(dmr_ms_alloc(c));
    }
    if (enable != c->dmr.ms.on) {
        // what the loop holds behind an MS / direct-mode word: dmrMSData()'s and dmrMS()'s counts, or the row's defaults again (with the
        // handlers on the counts serve no BS word)
        const int* def = ddn_fsk4::kRow[DDN_FSK4_DMR].lock_symbols;
        int32_t* lock = new (std::nothrow) int32_t[(size_t)c->B * 4];
        if (!lock) {
            return DDN_ENOMEM;
        }
        for (int i = 0; i < c->B; i++) {
            lock[4 * i] = enable ? DDN_DMR_MS_LOCK_DATA : def[0];
            lock[4 * i + 1] = enable ? DDN_DMR_MS_LOCK_VOICE : def[1];
            lock[4 * i + 2] = def[2];
            lock[4 * i + 3] = def[3];
        }
        const int rc = ddn_fsk4_rx_set_lock_symbols(c->rx, lock);
        delete[] lock;
        DDN_TRY(rc);
    }
    c->dmr.ms.on = enable;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_dmr_ms_results(ddn_fsk4_chain* c, ddn_dmr_ms_chain_results* r) {
    if (!c || !r || c->cfg.protocol != DDN_FSK4_DMR || !c->dmr.ms.on) {
        ddn_set_error("ddn_fsk4_chain_get_dmr_ms_results: a DMR chain with ddn_fsk4_chain_set_dmr_ms enabled");
        return DDN_EINVAL;
    }
    memset(r, 0, sizeof(*r));
    r->max_syncs = (size_t)c->myd;
    r->bursts = c->dmr.ms.b;
    r->data = c->dmr.ms.d;
    r->voice = c->dmr.ms.v;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_set_edacs_mode(ddn_fsk4_chain* c, int ea_mode, int esk_mask) {
    if (!c || c->cfg.protocol != DDN_FSK4_EDACS || (ea_mode != 0 && ea_mode != 1) || (esk_mask != 0 && esk_mask != 0xA0)) {
        ddn_set_error("ddn_fsk4_chain_set_edacs_mode: an EDACS chain, ea_mode 0 / 1 and esk_mask 0 / 0xA0 (-fh, -fH, -fe, -fE)");
        return DDN_EINVAL;
    }
    c->edacs.ea_mode = ea_mode;
    c->edacs.esk_mask = esk_mask;
    return DDN_OK;
}

extern "C" int
ddn_fsk4_chain_get_edacs_results(ddn_fsk4_chain* c, ddn_edacs_chain_results* r) {
    if (!c || !r || c->cfg.protocol != DDN_FSK4_EDACS) {
        ddn_set_error("ddn_fsk4_chain_get_edacs_results: not an EDACS chain");
        return DDN_EINVAL;
    }
    memset(r, 0, sizeof(*r));
    r->max_syncs = (size_t)c->myd;
    r->ea_mode = c->edacs.ea_mode;
    r->esk_mask = c->edacs.esk_mask;
    r->d_n_sync = c->d_ns;
    r->d_sync_pos = c->d_spos;
    r->d_sync_pat = c->d_spat;
    r->d_sync_thr5 = c->d_thr;
    r->d_raw40 = c->edacs.raw;
    r->d_vote40 = c->edacs.vote;
    r->d_bch_ok = c->edacs.bok;
    r->d_frame_ok = c->edacs.fok;
    r->d_msg28 = c->edacs.msg;
    r->d_kind = c->edacs.kind;
    r->d_types = c->edacs.types;
    r->d_site6 = c->edacs.site;
    r->d_valid = c->edacs.valid;
    return DDN_OK;
}

extern "C" void*
ddn_fsk4_chain_front_end(ddn_fsk4_chain* c) {
    return c ? c->fe : nullptr;
}
extern "C" void*
ddn_fsk4_chain_rx(ddn_fsk4_chain* c) {
    return c ? c->rx : nullptr;
}
