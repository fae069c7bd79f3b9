// ddn_api_chain_mixed.cpp - the mixed-protocol object over the three chains (include/ddn_chain.h): the P25 Phase 1, DMR and NXDN48
// groups of one batch (BASELINE configs[3]), their stages lined up across streams.  Host-only code.
#include <stdlib.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>

#include "ddn_chain_fsk4.h"
#include "ddn_device.h"
#include "ddn_hip.h"

struct ddn_mixed_chain {
    ddn_mixed_chain_config cfg;
    ddn_p25_chain* p25;
    ddn_fsk4_chain *dmr, *nxdn;
    hipStream_t st[3], st2[3]; // per group: front end + matched filter + loop / frame FEC + voice
    hipEvent_t ev_front[3], ev_loop[3], ev_dec[3];
    bool have_dec[3];
    // (round 5) front ends on streams of their own into two discriminator buffers per group: call k + 1's front end runs beside call
    // k's loop (ev_read[g][parity]: the loop that read that buffer has ended)
    bool overlap;
    hipStream_t stF[3];
    hipEvent_t ev_read[3][2];
    unsigned long long calls;
    // (round 6) one front-end launch for all the groups (ddn_batch_set_segments): the groups' channels share workgroups of sixteen, so a
    // 4096-channel mixed batch is one round of 256 workgroups instead of three launches of 171 eight-channel ones (two rounds and a half)
    ddn_batch* fe_all;
};

extern "C" void
ddn_mixed_chain_destroy(ddn_mixed_chain* m) {
    if (!m) {
        return;
    }
    (void)hipDeviceSynchronize();
    ddn_p25_chain_destroy(m->p25);
    ddn_fsk4_chain_destroy(m->dmr);
    ddn_fsk4_chain_destroy(m->nxdn);
    ddn_batch_destroy(m->fe_all);
    for (int k = 0; k < 3; k++) {
        for (hipStream_t s : {m->st[k], m->st2[k], m->stF[k]}) {
            if (s) {
                (void)hipStreamDestroy(s);
            }
        }
        for (hipEvent_t e : {m->ev_front[k], m->ev_loop[k], m->ev_dec[k], m->ev_read[k][0], m->ev_read[k][1]}) {
            if (e) {
                (void)hipEventDestroy(e);
            }
        }
    }
    delete m;
}

extern "C" int
ddn_mixed_chain_create(const ddn_mixed_chain_config* cfg, ddn_mixed_chain** out) {
    if (!cfg || !out || cfg->n_p25 < 0 || cfg->n_dmr < 0 || cfg->n_nxdn48 < 0 || cfg->n_p25 + cfg->n_dmr + cfg->n_nxdn48 <= 0
        || cfg->samples_per_call <= 0 || cfg->block_len <= 0) {
        ddn_set_error("ddn_mixed_chain_create: bad configuration");
        return DDN_EINVAL;
    }
    if (ddn_input_format_bytes(cfg->input_format) == 0) {
        ddn_set_error("ddn_mixed_chain_create: unknown input_format %d", cfg->input_format);
        return DDN_EINVAL;
    }
    *out = nullptr;
    ddn_mixed_chain* m = new (std::nothrow) ddn_mixed_chain();
    if (!m) {
        return DDN_ENOMEM;
    }
    memset(m, 0, sizeof(*m));
    m->cfg = *cfg;
    int rc = DDN_OK;
    if (cfg->n_p25 > 0) {
        ddn_p25_chain_config pc;
        memset(&pc, 0, sizeof(pc));
        pc.n_channels = cfg->n_p25;
        pc.samples_per_call = cfg->samples_per_call;
        pc.block_len = cfg->block_len;
        pc.input_format = cfg->input_format;
        pc.vocoder = cfg->vocoder;
        rc = ddn_p25_chain_create(&pc, &m->p25);
    }
    if (rc == DDN_OK && cfg->n_dmr > 0) {
        ddn_fsk4_chain_config dc = {cfg->n_dmr, cfg->samples_per_call, cfg->block_len, cfg->input_format, DDN_FSK4_DMR, 2, 0, 1,
                                    cfg->vocoder};
        rc = ddn_fsk4_chain_create(&dc, &m->dmr);
    }
    if (rc == DDN_OK && cfg->n_nxdn48 > 0) {
        ddn_fsk4_chain_config nc = {cfg->n_nxdn48, cfg->samples_per_call, cfg->block_len, cfg->input_format, DDN_FSK4_NXDN48, 0, 0, 1,
                                    cfg->vocoder};
        rc = ddn_fsk4_chain_create(&nc, &m->nxdn);
    }
    { // the three loops share the device: the DMR / NXDN48 kernels take the shape that suits the whole batch
        const int total = cfg->n_p25 + cfg->n_dmr + cfg->n_nxdn48;
        int cpw = 32;
        for (int c = 1; c <= 32; c *= 2) {
            if ((total + c - 1) / c <= 1536) {
                cpw = c;
                break;
            }
        }
        int cpw_d = cpw, cpw_n = cpw;
        // (experiments: values the setters reject are ignored, not passed on)
        auto pow2_1_32 = [](const char* e, int dflt) {
            const int v = e ? atoi(e) : 0;
            return (v >= 1 && v <= 32 && (v & (v - 1)) == 0) ? v : dflt;
        };
        {   // the overlapped schedule runs the fsk4 loops one channel per wavefront where a group allows it (<= 1536 channels: the
            // loop's fastest shape - 2.7 / 3.1 ms alone against 5.2 / 6.8 at four; the two loops then take turns on the device)
            const char* e = DDN_EXP_ENV("DDN_MIX_OVERLAP");
            if (cfg->overlap || (e && e[0] == '1')) {
                cpw_d = cfg->n_dmr <= 1536 ? 1 : cpw_d;
                cpw_n = cfg->n_nxdn48 <= 1536 ? 1 : cpw_n;
            }
        }
        cpw_d = pow2_1_32(DDN_EXP_ENV("DDN_MIX_CPW_DMR"), cpw_d);
        cpw_n = pow2_1_32(DDN_EXP_ENV("DDN_MIX_CPW_NXDN"), cpw_n);
        // Residency decides the step: a CU holds 8 of these wavefronts (~200 registers each).  At 4096 channels in thirds the P25
        // loop's own choice (4 channels per workgroup of 4 waves: 342 workgroups) + 2 x 342 two-wave workgroups are 2736 waves for
        // 2048 places - the loop launched last waits for the first to finish (measured: NXDN48 loop 9 ms, step 15.1 ms).  With 8
        // channels per P25 workgroup it is 2052 waves: step 14.2 ms.
        int cpw_p = (total > 2048 && (m->dmr || m->nxdn)) ? 8 : 0;
        if (const char* e = DDN_EXP_ENV("DDN_MIX_CPW_P25")) {
            const int v = atoi(e);
            if (v == 4 || v == 8 || v == 16 || v == 32 || v == 64) {
                cpw_p = v;
            }
        }
        if (rc == DDN_OK && m->p25 && cpw_p) {
            rc = ddn_p25_rx_set_channels_per_wave((ddn_p25_rx*)ddn_p25_chain_rx(m->p25), cpw_p);
        }
        if (rc == DDN_OK && m->dmr) {
            rc = ddn_fsk4_rx_set_channels_per_wave(m->dmr->rx, cpw_d);
        }
        if (rc == DDN_OK && m->nxdn) {
            rc = ddn_fsk4_rx_set_channels_per_wave(m->nxdn->rx, cpw_n);
        }
    }
    {   // cfg.overlap = 1 (off by default): front ends on streams of their own, two discriminator buffers per group - call k + 1's
        // front ends beside call k's loops.  Seven streams: it needs six or seven hardware queues per process (HIP's default
        // four hardware queues make streams share queues: 17-18 ms per step; with 6: 11.75 ms against 13.2 - profiles/README.md)
        const char* e = DDN_EXP_ENV("DDN_MIX_OVERLAP");
        m->overlap = cfg->overlap != 0 || (e && e[0] == '1');
    }
    if (rc == DDN_OK && m->overlap) {
        if (m->p25) {
            rc = ddn_p25_chain_double_disc(m->p25);
        }
        for (ddn_fsk4_chain* c : {m->dmr, m->nxdn}) {
            if (rc == DDN_OK && c && !c->d_disc2) {
                if (!c->pool.alloc(&c->d_disc2, (size_t)c->B * (size_t)c->n)) { // (the chain's own pool frees it with the chain)
                    rc = DDN_ENOMEM;
                }
            }
        }
        for (int k = 0; k < 3 && rc == DDN_OK; k++) {
            if (hipStreamCreateWithFlags(&m->stF[k], hipStreamNonBlocking) != hipSuccess
                || hipEventCreateWithFlags(&m->ev_read[k][0], hipEventDisableTiming) != hipSuccess
                || hipEventCreateWithFlags(&m->ev_read[k][1], hipEventDisableTiming) != hipSuccess) {
                rc = DDN_EHIP;
            }
        }
    }
    // DDN_MIX_XCD="a,b,c" (experiment): the three groups' loop streams on disjoint sets of XCDs (a + b + c <= 8; CU-mask bit i is
    // CU i / 8 of XCD i % 8) - different loop kernels then never share a CU's instruction cache
    int xcd_n[3] = {0, 0, 0};
    if (const char* e = DDN_EXP_ENV("DDN_MIX_XCD")) {
        if (sscanf(e, "%d,%d,%d", &xcd_n[0], &xcd_n[1], &xcd_n[2]) != 3 || xcd_n[0] < 1 || xcd_n[1] < 1 || xcd_n[2] < 1
            || xcd_n[0] + xcd_n[1] + xcd_n[2] > 8) {
            xcd_n[0] = xcd_n[1] = xcd_n[2] = 0;
        }
    }
    for (int k = 0, x0 = 0; k < 3 && rc == DDN_OK; k++) {
        hipError_t se;
        if (xcd_n[k]) {
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < 256; i++) {
                if (i % 8 >= x0 && i % 8 < x0 + xcd_n[k]) {
                    mask[i / 32] |= 1u << (i % 32);
                }
            }
            x0 += xcd_n[k];
            se = hipExtStreamCreateWithCUMask(&m->st[k], 8, mask);
        } else {
            se = hipStreamCreateWithFlags(&m->st[k], hipStreamNonBlocking);
        }
        if (se != hipSuccess
            || (k == 0 && hipStreamCreateWithFlags(&m->st2[0], hipStreamNonBlocking) != hipSuccess)
            || hipEventCreateWithFlags(&m->ev_front[k], hipEventDisableTiming) != hipSuccess
            || hipEventCreateWithFlags(&m->ev_loop[k], hipEventDisableTiming) != hipSuccess
            || hipEventCreateWithFlags(&m->ev_dec[k], hipEventDisableTiming) != hipSuccess) {
            rc = DDN_EHIP;
        }
    }
    if (rc == DDN_OK && !m->overlap && (m->p25 != nullptr) + (m->dmr != nullptr) + (m->nxdn != nullptr) >= 2) {
        // the shared front end: one batch object over all channels, a segment per group present (the profiles the groups' own chain
        // objects design: P25 C4FM / 12.5 kHz / 6.25 kHz - all 135 taps at 48 kHz; a set of profiles with different tap counts
        // keeps the groups' own front ends)
        int32_t cnt[3], prof[3];
        int ns = 0;
        const int gcnt[3] = {cfg->n_p25, cfg->n_dmr, cfg->n_nxdn48}, gprof[3] = {DDN_LPF_P25_C4FM, DDN_LPF_12K5, DDN_LPF_6K25};
        for (int g = 0; g < 3; g++) {
            if (gcnt[g] > 0) {
                cnt[ns] = gcnt[g];
                prof[ns++] = gprof[g];
            }
        }
        ddn_front_end_config fc = {cfg->n_p25 + cfg->n_dmr + cfg->n_nxdn48, 48000, 4800, 4, prof[0], cfg->input_format, cfg->block_len, 0.0f};
        if (!DDN_EXP_ENV("DDN_MIX_OWN_FE") && ddn_batch_create(&fc, &m->fe_all) == DDN_OK) {
            if (ddn_batch_set_segments(m->fe_all, ns, cnt, prof) != DDN_OK || cfg->samples_per_call < DDN_CARRY_LEN) {
                ddn_batch_destroy(m->fe_all);
                m->fe_all = nullptr;
            }
        }
    }
    if (rc != DDN_OK) {
        ddn_mixed_chain_destroy(m);
        return rc;
    }
    *out = m;
    return DDN_OK;
}

extern "C" int
ddn_mixed_chain_run(ddn_mixed_chain* m, const void* d_iq_p25, const void* d_iq_dmr, const void* d_iq_nxdn48) {
    if (!m || (m->p25 && !d_iq_p25) || (m->dmr && !d_iq_dmr) || (m->nxdn && !d_iq_nxdn48)) {
        return DDN_EINVAL;
    }
    // The protocol groups are independent channel sets, two streams each.  Their stages are lined up across the groups: the three
    // front ends first (kernels that would otherwise be starved by - and delay the workgroups of - another group's receive loop),
    // then the three receive loops side by side (latency chains that fit on the device together).  A group's frame FEC / voice stage
    // runs on its second stream behind its loop, so the NEXT call's front end does not queue up behind it (a front end of <= 2048
    // channels is a 3 ms latency chain whatever the batch: what it runs beside costs it little) - the next call's loop waits for it
    // (the loop's sync lists, handler events and payload rows are single buffers the decode stage reads).
    const void* iq[3] = {d_iq_p25, d_iq_dmr, d_iq_nxdn48};
    const bool on[3] = {m->p25 != nullptr, m->dmr != nullptr, m->nxdn != nullptr};
    auto stage = [&](int g, int st_no) -> int {
        // (one decode stream for the three groups: HIP maps streams onto four hardware queues, a fifth stream would share a queue
        // with one of the loops - measured: the NXDN48 loop then ran behind the P25 loop)
        hipStream_t s = st_no == 2 ? m->st2[0] : m->st[g];
        if (g == 0) {
            return ddn_p25_chain_stage(m->p25, st_no, iq[0], s);
        }
        return ddn_fsk4_chain_stage(g == 1 ? m->dmr : m->nxdn, st_no, iq[g], s);
    };
    // (round 5, measured and left off) DDN_MIX_PHASED=1: a call's front ends start when ALL loops of the call before have ended
    // instead of each behind its own group's loop (where it crawls beside the other groups' loops, 4-5 ms).  Lined up, the three
    // front ends take ~3 ms together, but the loops then have nothing beside them either: 14.4-15.4 ms per step against 13.2.
    static const bool phased = [] {
        const char* e = DDN_EXP_ENV("DDN_MIX_PHASED");
        return e && e[0] == '1';
    }();
    // (the discriminator buffer a group's call uses is picked by that chain's own step parity, the event that guards it by m->calls'.
    // A part-level flush through ddn_mixed_chain_part() advances the part's step and shifts the two against each other; it also
    // synchronises everything first, so the call after it has no reader to wait for, and from the call after that the event waited
    // for is that of a LATER loop than the buffer's last reader - an over-wait, never a race)
    const int par = (int)(m->calls & 1);
    if (m->overlap) {
        // (round 5) A group is a chain front end -> matched filter -> loop, and with one discriminator buffer the step could not be
        // shorter than the slowest group's chain (NXDN48: 4.4 + 1.4 + 6.8 ms).  With two buffers and the front ends on streams of
        // their own, call k + 1's front end runs beside call k's loop (the host runs ahead); it waits for the loop that read its
        // buffer two calls ago.  The carried record tails are copied at the head of stage 1, so stage 0 touches nothing a loop writes.
        for (int g = 0; g < 3; g++) {
            if (on[g]) {
                if (m->calls >= 2) {
                    HIP_TRY(hipStreamWaitEvent(m->stF[g], m->ev_read[g][par], 0));
                }
                if (g == 0) {
                    DDN_TRY(ddn_p25_chain_stage(m->p25, 0, iq[0], m->stF[0]));
                } else {
                    DDN_TRY(ddn_fsk4_chain_stage(g == 1 ? m->dmr : m->nxdn, 0, iq[g], m->stF[g]));
                }
                HIP_TRY(hipEventRecord(m->ev_front[g], m->stF[g]));
            }
        }
        for (int g = 0; g < 3; g++) {
            if (!on[g]) {
                continue;
            }
            HIP_TRY(hipStreamWaitEvent(m->st[g], m->ev_front[g], 0));
            if (m->have_dec[g]) {
                HIP_TRY(hipStreamWaitEvent(m->st[g], m->ev_dec[g], 0));
            }
            DDN_TRY(stage(g, 1));
            HIP_TRY(hipEventRecord(m->ev_loop[g], m->st[g]));
            HIP_TRY(hipEventRecord(m->ev_read[g][par], m->st[g]));
        }
    } else if (m->fe_all) {
        // one front-end launch for every group.  It writes every group's discriminator buffer, so it waits for all the loops of the
        // call before; every group's matched filter + loop then follows it on the group's stream.  It goes on the stream of the
        // LAST group present - the loop that ends last (NXDN48 6 ms, DMR 5, P25 4.8 side by side): queued right behind that loop
        // it is dispatched the moment the loop ends.  On another stream it is released by an event, in a race with that group's
        // decode stage (released by the same event), whose many small workgroups keep taking a little LDS on every CU while a front-end
        // workgroup needs a CU's whole LDS: measured 4.0 ms for the launch instead of 2.2.
        const int g0 = on[2] ? 2 : (on[1] ? 1 : 0);
        hipStream_t sf = m->st[g0];
        for (int g = 0; g < 3; g++) {
            if (on[g] && g != g0 && m->calls > 0) {
                HIP_TRY(hipStreamWaitEvent(sf, m->ev_loop[g], 0));
            }
        }
        const void* in[3];
        float* disc[3];
        int ns = 0;
        if (on[0]) {
            DDN_TRY(ddn_p25_chain_stage0_prepare(m->p25, sf, &disc[ns]));
            in[ns++] = iq[0];
        }
        if (on[1]) {
            disc[ns] = ddn_fsk4_chain_disc_buffer(m->dmr);
            in[ns++] = iq[1];
        }
        if (on[2]) {
            disc[ns] = ddn_fsk4_chain_disc_buffer(m->nxdn);
            in[ns++] = iq[2];
        }
        DDN_TRY(ddn_front_end_run_segments(m->fe_all, in, (size_t)m->cfg.samples_per_call, disc, sf));
        HIP_TRY(hipEventRecord(m->ev_front[g0], sf));
        for (int g = 0; g < 3; g++) {
            if (!on[g]) {
                continue;
            }
            if (g != g0) {
                HIP_TRY(hipStreamWaitEvent(m->st[g], m->ev_front[g0], 0));
            }
            if (m->have_dec[g]) {
                // the loop overwrites what the decode stage of the call before reads of it: P25 - the whole stage (its records and
                // events are triple-buffered, but a loop that starts beside LDS-hungry decode kernels is slowed for its whole
                // length); DMR / NXDN48 - the stage's gathers only (their loop's sync lists and events are single buffers), the
                // frame FEC and synthesis behind them run on beside the loop
                hipEvent_t gate = g == 0 ? m->ev_dec[0] : (hipEvent_t)ddn_fsk4_chain_reads_done_event(g == 1 ? m->dmr : m->nxdn);
                HIP_TRY(hipStreamWaitEvent(m->st[g], gate, 0));
            }
            DDN_TRY(stage(g, 1));
            HIP_TRY(hipEventRecord(m->ev_loop[g], m->st[g]));
        }
    } else {
    for (int g = 0; g < 3; g++) {
        if (on[g]) {
            if (phased) {
                for (int h = 0; h < 3; h++) {
                    if (h != g && on[h] && m->have_dec[h]) { // (have_dec: the group's events have been recorded once)
                        HIP_TRY(hipStreamWaitEvent(m->st[g], m->ev_loop[h], 0));
                    }
                }
            }
            DDN_TRY(stage(g, 0));
            HIP_TRY(hipEventRecord(m->ev_front[g], m->st[g]));
        }
    }
    for (int g = 0; g < 3; g++) {
        if (!on[g]) {
            continue;
        }
        for (int h = 0; h < 3; h++) {
            if (h != g && on[h]) {
                HIP_TRY(hipStreamWaitEvent(m->st[g], m->ev_front[h], 0));
            }
        }
        if (m->have_dec[g]) {
            HIP_TRY(hipStreamWaitEvent(m->st[g], m->ev_dec[g], 0));
        }
        DDN_TRY(stage(g, 1));
        HIP_TRY(hipEventRecord(m->ev_loop[g], m->st[g]));
    }
    }
    m->calls++;
    if (m->fe_all && !m->overlap) {
        // (round 6) With one decode stream for the three groups that stream was the step: its kernels run beside the front end and
        // the loops at a fraction of their speed (k_p25_lsd 1.6 ms for 0.05, k_mbe_synth 2 ms for 0.5), one group after the other -
        // 11.6 of a 12.5 ms step busy, whatever the front end and the loops did.  Now a group's decode stage follows its loop on the
        // loop's own stream (it runs beside the loops that are still going; the group's next loop comes behind the shared front
        // end anyway) - except the last group's, whose stream carries the front end of the next call right behind its loop: its
        // decode goes to the decode stream, beside that front end.
        const int g0 = on[2] ? 2 : (on[1] ? 1 : 0);
        for (int g = 0; g < 3; g++) {
            if (on[g]) {
                hipStream_t sd = g == g0 ? m->st2[0] : m->st[g];
                if (g == g0) {
                    HIP_TRY(hipStreamWaitEvent(sd, m->ev_loop[g], 0));
                }
                DDN_TRY(g == 0 ? ddn_p25_chain_stage(m->p25, 2, iq[0], sd) : ddn_fsk4_chain_stage(g == 1 ? m->dmr : m->nxdn, 2, iq[g], sd));
                HIP_TRY(hipEventRecord(m->ev_dec[g], sd));
                m->have_dec[g] = true;
            }
        }
        return DDN_OK;
    }
    for (int g = 0; g < 3; g++) {
        if (on[g]) {
            HIP_TRY(hipStreamWaitEvent(m->st2[0], m->ev_loop[g], 0));
            DDN_TRY(stage(g, 2));
            HIP_TRY(hipEventRecord(m->ev_dec[g], m->st2[0]));
            m->have_dec[g] = true;
        }
    }
    return DDN_OK;
}

extern "C" int
ddn_mixed_chain_wait(ddn_mixed_chain* m) {
    if (!m) {
        return DDN_EINVAL;
    }
    for (int k = 0; k < 3; k++) {
        if (m->stF[k]) {
            HIP_TRY(hipStreamSynchronize(m->stF[k]));
        }
        HIP_TRY(hipStreamSynchronize(m->st[k]));
        if (m->st2[k]) {
            HIP_TRY(hipStreamSynchronize(m->st2[k]));
        }
    }
    return DDN_OK;
}

extern "C" void*
ddn_mixed_chain_part(ddn_mixed_chain* m, int which) {
    if (!m) {
        return nullptr;
    }
    return which == 0 ? (void*)m->p25 : (which == 1 ? (void*)m->dmr : (which == 2 ? (void*)m->nxdn : nullptr));
}

// Block partition of a mixed batch over the ranks of a node: the global channel index is [P25 | DMR | NXDN48]; rank
// r of `world` owns a contiguous block of it (the first total % world ranks one channel more) and therefore a contiguous range of
// each protocol group.  Pure arithmetic: every rank computes the same table.
extern "C" int
ddn_mixed_partition(int n_p25, int n_dmr, int n_nxdn48, int rank, int world, int32_t first3[3], int32_t count3[3]) {
    if (n_p25 < 0 || n_dmr < 0 || n_nxdn48 < 0 || world <= 0 || rank < 0 || rank >= world || !first3 || !count3) {
        return DDN_EINVAL;
    }
    const long total = (long)n_p25 + n_dmr + n_nxdn48;
    const long base = total / world, extra = total % world;
    const long lo = rank * base + (rank < extra ? rank : extra), hi = lo + base + (rank < extra ? 1 : 0);
    const long start[3] = {0, n_p25, (long)n_p25 + n_dmr}, len[3] = {n_p25, n_dmr, n_nxdn48};
    for (int k = 0; k < 3; k++) {
        const long a = lo > start[k] ? lo : start[k], b = hi < start[k] + len[k] ? hi : start[k] + len[k];
        first3[k] = (int32_t)(b > a ? a - start[k] : 0);
        count3[k] = (int32_t)(b > a ? b - a : 0);
    }
    return DDN_OK;
}
