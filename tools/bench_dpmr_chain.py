#!/usr/bin/env python3
"""The dPMR chain object (ddn_fsk4_chain, protocol DDN_FSK4_DPMR, -fm, vocoder = 1) at batch scale, for rocprofv3 --kernel-trace --stats:
1365 and 4096 channels x 48 000 cu8 samples of the reference's dPMR capture, every channel a different rotation, I/Q resident, one C
call per step.  The capture is sent inverted: plain -fm locks on a handful of its superframes (the reference's "Src=1601621"), the
I/Q-swapped capture on every one (the -xd reading: TG = Src = 3939*5*, channel code 2, voice).  Even channels carry the capture as
sent, odd channels swapped.  Known answers are read off the device outputs of the first call before the timed steps; one JSON line.
usage: bench_dpmr_chain.py [--steps K]"""
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


def dpmr_chain(B, n, steps):
    from conftest import golden
    dev = torch.device("cuda")
    iq = torch.from_numpy(np.ascontiguousarray(golden("iq_dpmr.npz")["iq"], np.uint8)).to(dev)
    m = iq.shape[0]
    off = (torch.arange(B, device=dev) * 9973) % (m - n)
    x = iq[off[:, None] + torch.arange(n, device=dev)[None, :]].contiguous()
    x[1::2] = x[1::2].flip(-1).contiguous()
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DPMR, rf_mod=2, handlers=0, vocoder=1)
    ch.run(x.data_ptr())          # (the known answers are read off this first call: replaying the buffer puts a seam into the stream)
    torch.cuda.synchronize()
    r = ch.dpmr_results()
    S = r.max_syncs
    ns = ch.fetch(r.d_n_sync, np.int32, (B,))
    sel = np.arange(S)[None, :] < ns[:, None]
    odd = (np.arange(B)[:, None] % 2 == 1) & sel
    even = (np.arange(B)[:, None] % 2 == 0) & sel
    valid = ch.fetch(r.d_valid, np.uint8, (B, S))
    crc = ch.fetch(r.d_crc_ok2, np.uint8, (B, S, 2)).all(axis=2) & (valid == 1)
    color = ch.fetch(r.d_color, np.int32, (B, S))
    src = ch.fetch(r.d_src, np.int32, (B, S))
    tg = ch.fetch(r.d_tg, np.int32, (B, S))
    nv = ch.fetch(r.d_n_voice, np.int32, (B,))
    name = lambda vals: sorted({ddn.dpmr_air_interface_id(v) for v in vals if v >= 0})
    out = {"channels": B, "superframes_decoded": int(valid[sel].sum()),
           "swapped_channels": {"superframes": int(valid[odd].sum()), "both_crc_good": int(crc[odd].sum()),
                                "channel_codes_of_crc_good": sorted({int(v) for v in color[odd & crc]}),
                                "published_tg": name(tg[odd]), "published_src": name(src[odd])},
           "as_sent_channels": {"superframes": int(valid[even].sum()), "published_src": name(src[even])[:4],
                                "src_1601621_published": "1601621" in name(src[even])},
           "voice_frames_synthesized": int(nv.sum())}
    ch.run(x.data_ptr())
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
    res = {"workload": "channels x %d cu8 samples of the reference's dPMR capture (rotated per channel), -fm, vocoder = 1, one C call "
                       "per step" % n, "device": torch.cuda.get_device_name(0)}
    for B in (1365, 4096):
        res["%d_channels" % B] = dpmr_chain(B, n, a.steps)
    print(json.dumps({"dpmr_chain": res}))


if __name__ == "__main__":
    main()
