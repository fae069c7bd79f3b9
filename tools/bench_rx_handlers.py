#!/usr/bin/env python3
"""Receive-loop kernel time on the bench traffic (4096 channels x 48000 samples, half voice half control): configured in-frame
lengths (the round-2 shape) against the reference's handlers inside the loop, per lanes-per-wave choice.
usage: [MODES=handlers:8,...] [TRAFFIC=mixed,voice,ctrl] [DDN_RX_DBG=flags,flags,...] [STEPS=k] python tools/bench_rx_handlers.py [B] [n]
With DDN_RX_DBG bit 8192 and a library built with -DDDN_RX_CYCLES=1 (DDN_LIB_PATH): the cycle tables of both recurrence waves, the
staging wave and the handler wave."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsd-neo_amd", "bindings"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import ddn

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
n = int(sys.argv[2]) if len(sys.argv) > 2 else 48000
voice, ctrl = bench.make_base_traffic(n)
fe = ddn.Batch(B, block_len=8192)
disc = torch.zeros((B, n), dtype=torch.float32, device="cuda")
l = ddn.lib()
# TRAFFIC and DDN_RX_DBG may be comma-separated lists: every combination runs in this one process, on the same generated traffic
# (TRAFFIC: mixed = the bench's half voice half control, voice / ctrl = one kind of channel only)
MODES = [(m, int(c)) for m, c in (x.split(":") for x in os.environ.get("MODES", "locks:8,handlers:8,handlers:16,locks:16").split(","))]
RUNS = [(tr, int(d, 0), m, c) for tr in os.environ.get("TRAFFIC", "mixed").split(",") for d in os.environ.get("DDN_RX_DBG", "0").split(",")
        for m, c in MODES]
STEPS = int(os.environ.get("STEPS", "6"))   # the loop's time is the mean over the steps after the third
cur_traffic = None
for traffic, DBG, mode, cpw in RUNS:
    if traffic != cur_traffic:
        cur_traffic = traffic
        idx = [bench.channel_source(c) for c in range(B)]
        if traffic in ("voice", "ctrl"):
            idx = [(traffic, i) for _, i in idx]
        d_iq = torch.from_numpy(np.stack([(voice if k == "voice" else ctrl)[i] for k, i in idx])).cuda()
        locks = np.array([840 if k == "voice" else int(os.environ.get("LOCK_CC", "156")) for k, _ in idx], np.int32)
    # (the product library reads no environment: the schedule selectors and the filter-in-the-loop switch go through the setters)
    rx = ddn.P25Rx(B, use_matched_filter=1, channels_per_wave=cpw, handlers=(mode == "handlers"),
                   debug_flags=((DBG + 2**31) % 2**32) - 2**31,  # (bit 31 = the int's sign)
                   filter_in_loop=os.environ.get("FIL", "0") == "1")
    if mode == "locks":
        assert l.ddn_p25_rx_set_lock_symbols(rx.h, locks.ctypes.data) == 0
    ms = l.ddn_p25_rx_max_symbols(rx.h, n)
    rec = torch.zeros((B, ms, 10), dtype=torch.uint8, device="cuda")
    fl = torch.zeros((B, ms), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ev = torch.zeros((B, 256, 4), dtype=torch.int32, device="cuda")
    nev = torch.zeros((B,), dtype=torch.int32, device="cuda")
    if mode == "handlers":
        assert l.ddn_p25_rx_set_events(rx.h, ev.data_ptr(), nev.data_ptr(), 256) == 0
    assert l.ddn_p25_rx_set_timing(rx.h, 1) == 0
    for step in range(STEPS):
        fe.run_device(d_iq.data_ptr(), n, disc.data_ptr(), None)
        assert l.ddn_p25_rx_run(rx.h, disc.data_ptr(), n, rec.data_ptr(), fl.data_ptr(), cnt.data_ptr(), ms, None) == 0
        torch.cuda.synchronize()
        if step == 2:
            assert l.ddn_p25_rx_set_timing(rx.h, 1) == 0
    t = (C.c_float * 2)()
    k = C.c_int()
    assert l.ddn_p25_rx_get_timing_avg(rx.h, t, C.byref(k)) == 0
    flc = fl.cpu().numpy()
    extra = ""
    if mode == "handlers":
        e = ev.cpu().numpy()
        ne = nev.cpu().numpy()
        allev = np.concatenate([e[c, :min(ne[c], 256)] for c in range(B)])
        if DBG & 131072:
            for kd in (1, 2):
                a = allev[(allev[:, 1] == kd) & ((allev[:, 2] & 15) == 0)]
                extra += " | kind %d stamps(cycles): %.0f %.0f %.0f" % (kd, (a[:, 2] >> 4).mean() * 16, (a[:, 3] & 0xFFFF).mean() * 16,
                                                                      ((a[:, 3] >> 16) & 0xFFFF).mean() * 16)
        elif DBG & 1073741824:  # DDN_RX_CYCLES build: e[2] = cycles the request lay unserved
            for kd in (1, 2):
                a = allev[allev[:, 1] == kd]
                extra += " | kind %d: pick-up delay mean %.0f pct[10,50,80,90,95,99] %s, service mean %.0f" % (
                    kd, a[:, 2].mean(), np.percentile(a[:, 2], [10, 50, 80, 90, 95, 99]).astype(int).tolist(), a[:, 3].mean())
        elif DBG & 65536:
            for kd in (1, 2):
                a = allev[allev[:, 1] == kd]
                for path in (0, 1):
                    v = a[a[:, 2] == path][:, 3]
                    if len(v):
                        extra += " | kind %d path %d: n %d cycles mean %.0f max %d" % (kd, path, len(v), v.mean(), v.max())
                        extra += " pct[10,50,80,90,95,99] %s" % np.percentile(v, [10, 50, 80, 90, 95, 99]).astype(int).tolist()
        else:
            extra = " events/ch %.1f nid_ok %.3f tsbk_crc %.3f" % (ne.mean(), (allev[allev[:, 1] == 1][:, 2] > 0).mean(),
                                                                   (allev[allev[:, 1] == 2][:, 3] & 1).mean())
    if mode == "handlers" and DBG & 65536:
        tot = np.zeros(2)
        for c in range(0, 64):
            o = (C.c_longlong * 2)()
            assert l.ddn_p25_rx_debug_counters(rx.h, c, o) == 0
            tot += [o[0], o[1]]
        extra += " | lane wait: %.0f cycles per request (%d requests)" % (tot[1] / max(tot[0], 1), tot[0])
    if DBG & 8192:      # library built with EXTRA=-DDDN_RX_CYCLES=1
        r = rec.cpu().numpy().reshape(B, -1)
        tiles = (n + 127) // 128
        nwg = len(range(0, B, cpw))

        def block(off):   # the 64-byte block that ends `off` bytes above the end of each workgroup's first record area, as int64[8]
            return np.stack([r[c, r.shape[1] - off - 64:r.shape[1] - off] for c in range(0, B, cpw)]).copy().view(np.int64)

        # the kernel's layout (ddn_rx.hip, end of k_p25_rxw): busy / wait blocks of recurrence 0, recurrence 1 and the staging wave
        # (plain mode: recurrence, -, loader + winprep); then per recurrence wave w a bank 640 * w bytes further down
        hm_mode = mode == "handlers"
        roles = [("recurrence 0", 128), ("recurrence 1", 64), ("staging", 0)] if hm_mode else [("recurrence", 128), ("loader / winprep", 0)]
        for nm, off in roles:
            v = block(off)
            tot = (v[:, 0] + v[:, 1]) / tiles
            extra += "\n   %-12s busy/tile %.0f wait/tile %.0f cycles; busy + wait over workgroups: mean %.0f p95 %.0f max %.0f" % (
                nm, v[:, 0].mean() / tiles, v[:, 1].mean() / tiles, tot.mean(), np.percentile(tot, 95), tot.max())
        st = block(0)
        extra += "\n   staging wave per tile (both halves): stage %.0f drain %.0f window summaries %.0f cycles" % tuple(
            st[:, 2 + k].mean() / tiles for k in range(3))
        for w in range(2 if hm_mode else 1):
            bank = 640 * w
            tt = block(128 - 64 * w)
            extra += "\n  -- recurrence %d" % w
            for k in range(3):
                extra += "\n   trip kind %d: %.2f per tile at %.0f cycles (share of busy %.2f)" % (
                    k, tt[:, 5 + k].mean() / tiles, tt[:, 2 + k].sum() / max(1, tt[:, 5 + k].sum()), tt[:, 2 + k].sum() / max(1, tt[:, 0].sum()))
            sec = block(192 + bank)
            nstd = max(1, tt[:, 5].sum())
            extra += "\n   std trip sections (cycles per trip): top %.0f search %.0f mean %.0f inframe %.0f hunt %.0f emit %.0f" % tuple(
                sec[:, k].sum() / nstd for k in range(6))
            extra += "\n   bulk hunting passes: %.2f per tile at %.0f cycles" % (sec[:, 7].sum() / (nwg * tiles), sec[:, 6].sum() / max(1, sec[:, 7].sum()))
            blk = block(320 + bank).sum(axis=0)
            extra += "\n   bulk pass per owner lane (%.2f owners per pass, %.1f symbols each): set-up %.0f masks + slip chain %.0f means + sync test %.0f stores %.0f window reduction %.0f owner's words %.0f cycles" % (
                (blk[7] / max(1, sec[:, 7].sum()), blk[6] / max(1, blk[7])) + tuple(blk[k] / max(1, blk[7]) for k in range(6)))
            blk2 = block(512 + bank).sum(axis=0)
            if blk2[0] > 0:    # two / four lanes per recurrence wave: the middle part split, and how many passes had several owners
                extra += "\n   of that, masks %.0f slip chain %.0f cycles; %.2f of the passes had several owners" % (
                    blk2[0] / max(1, blk[7]), (blk[1] - blk2[0]) / max(1, blk[7]), blk2[1] / max(1, sec[:, 7].sum()))
            run = block(256 + bank).sum(axis=0)
            extra += "\n   lean runs: %.2f per tile, %.2f trips and %.2f phases each (%.2f of them polling a handler mailbox), %.0f cycles inside the run per trip" % (
                run[0] / (nwg * tiles), run[1] / max(1, run[0]), run[7] / max(1, run[0]), run[5] / max(1, run[0]), run[6] / max(1, run[1]))
            extra += "\n   a lean run's pass: %.0f cycles from the pass's top to the bulk test's end, %.0f from there to the run's first trip" % (
                run[2] / max(1, run[0]), run[3] / max(1, run[0]))
            ent = block(448 + bank).sum(axis=0)
            extra += "\n   that entry by part: queue hand-over %.0f, lean tests + entry proof %.0f, run length %.0f cycles" % tuple(
                ent[k] / max(1, run[0]) for k in range(3))
            if hm_mode:
                hw = block(576 + bank).sum(axis=0)
                extra += "\n   with a lane waiting for its handler: %.0f cycles per tile in %.2f passes, %.2f of them found an answer" % (
                    hw[0] / (nwg * tiles), hw[1] / (nwg * tiles), hw[2] / (nwg * tiles))
        if hm_mode:
            hm = block(384).sum(axis=0)
            extra += "\n   handler wave per tile: filter passes %.2f at %.0f cycles, decisions %.2f at %.0f cycles, idle polls %.1f" % (
                hm[1] / (nwg * tiles), hm[0] / max(1, hm[1]), hm[3] / (nwg * tiles), hm[2] / max(1, hm[3]), hm[4] / (nwg * tiles))
    print("%-5s dbg %d %-8s cpw %2d: loop %.3f ms (mf %.3f) in-frame share %.3f syncs/ch %.1f%s" % (
        traffic, DBG, mode, cpw, t[1], t[0], (flc & 1).mean() * ms / (n / 10), (flc & 2).sum() / B, extra), flush=True)
