#!/usr/bin/env python3
"""The D-STAR chain object (ddn_fsk4_chain, protocol DDN_FSK4_DSTAR, -fd, vocoder = 0) at batch scale, for rocprofv3 --kernel-trace --stats:
1365 and 4096 channels x 48 000 cu8 samples of the reference's D-STAR capture, every channel a different rotation, I/Q resident, one C
call per step.  Even channels carry the capture as sent (the positive words), odd channels I/Q-swapped (the negative words).  The units
decoded and the slow-data headers read are taken off the device outputs of the first calls before the timed steps; one JSON line.
usage: bench_dstar_chain.py [--steps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsd-neo_amd", "bindings"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import ddn


def dstar_chain(B, n, steps):
    from conftest import golden
    dev = torch.device("cuda")
    iq = torch.from_numpy(np.ascontiguousarray(golden("iq_dstar.npz")["iq"], np.uint8)).to(dev)
    m = iq.shape[0]
    off = (torch.arange(B, device=dev) * 9973) % (m - n)
    x = iq[off[:, None] + torch.arange(n, device=dev)[None, :]].contiguous()
    x[1::2] = x[1::2].flip(-1).contiguous()
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DSTAR, rf_mod=2, handlers=0, vocoder=0)
    units = hdr_ok = sd_hdr_ok = 0
    srcs = set()
    for _ in range(2):            # (a unit is decoded once the carry behind its sync has arrived: the second call decodes the first's)
        ch.run(x.data_ptr())
        torch.cuda.synchronize()
        r = ch.dstar_results()
        S = r.max_syncs
        ns = ch.fetch(r.d_n_sync, np.int32, (B,))
        sel = np.arange(S)[None, :] < ns[:, None]
        valid = ch.fetch(r.d_valid, np.uint8, (B, S)).astype(bool) & sel
        hv = ch.fetch(r.d_hdr_valid, np.uint8, (B, S)).astype(bool) & sel
        hok = ch.fetch(r.d_hdr_crc_ok, np.uint8, (B, S)).astype(bool) & hv
        kind = ch.fetch(r.d_sd_kind, np.uint8, (B, S))
        sok = ch.fetch(r.d_sd_crc_ok, np.uint8, (B, S)).astype(bool) & valid & (kind == 1)
        sh = ch.fetch(r.d_sd_hdr41, np.uint8, (B, S, 41))
        units += int(valid.sum())
        hdr_ok += int(hok.sum())
        sd_hdr_ok += int(sok.sum())
        srcs |= {bytes(sh[c, k, 27:39]).decode("latin-1") for c, k in zip(*np.nonzero(sok))}
    out = {"channels": B, "units_decoded_two_calls": units, "radio_headers_crc_good": hdr_ok, "slow_data_headers_crc_good": sd_hdr_ok,
           "slow_data_src": sorted(srcs)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        ch.run(x.data_ptr())
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    out.update({"ms_per_step": round(ms, 3), "Msamples_per_s": round(B * n / ms / 1e3, 1)})
    ch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    n = 48000
    res = {"workload": "channels x %d cu8 samples of the reference's D-STAR capture (rotated per channel, odd channels I/Q-swapped), -fd, "
                       "one C call per step" % n, "device": torch.cuda.get_device_name(0)}
    for B in (1365, 4096):
        res["%d_channels" % B] = dstar_chain(B, n, a.steps)
    print(json.dumps({"dstar_chain": res}))


if __name__ == "__main__":
    main()
