#!/usr/bin/env python3
"""EDACS chain benchmark: the fsk4 chain object (DDN_FSK4_EDACS, -fh) from cu8 I/Q on one GPU - front end, 9600-baud receive loop,
the control-channel frame decode - on the reference's EDACS capture rotated per channel (odd channels I/Q-swapped: the +EDACS words),
48 000 samples per call (1 s at 48 ksps).  Prints one JSON line: per batch size the median ms per call and the realtime factor.

    python3 tools/bench_edacs_chain.py [--channels 1365,4096] [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsd-neo_amd", "bindings"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="1365,4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import ddn
    g = np.load(os.path.join(ROOT, "tests", "golden", "iq_edacs.npz"))
    iq = np.ascontiguousarray(g["iq"], np.uint8)
    n = 48000
    out = {"bench": "edacs_chain", "samples_per_call": n, "rf_mod": 2, "mode": "-fh", "results": []}
    for B in [int(v) for v in a.channels.split(",")]:
        x = np.empty((B, n, 2), np.uint8)
        for c in range(B):
            r = np.roll(iq, (c * 2851) % len(iq), axis=0)[:n]
            x[c] = r[:, ::-1] if c & 1 else r
        d = torch.from_numpy(x).cuda()
        ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_EDACS, rf_mod=2, handlers=0, vocoder=0)
        ch.set_edacs_mode(0, 0)
        for _ in range(a.warmup):
            ch.run(d.data_ptr())
        torch.cuda.synchronize()
        times = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            ch.run(d.data_ptr())
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        rd = ch.edacs_results()
        ns = ch.fetch(rd.d_n_sync, np.int32, (B,))
        kind = ch.fetch(rd.d_kind, np.uint8, (B, rd.max_syncs))
        ms = float(np.median(times))
        out["results"].append({"channels": B, "ms_per_call": round(ms, 3), "ms_min": round(float(np.min(times)), 3),
                               "realtime_x": round(1000.0 / ms, 1), "frames_last_call": int(ns.sum()),
                               "site_id_frames_last_call": int((kind == 3).sum())})
        ch.close()
        del d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
