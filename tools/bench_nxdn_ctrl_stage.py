"""What decoding NXDN control and data channels on the device costs: an NXDN96 chain's whole step (ddn_fsk4_chain_stage 0, 1, 2) and
its stage 2 alone (frame gather, SACCH / FACCH1 decodes and - once ddn_fsk4_chain_set_nxdn_ctrl has been called - the CAC / FACCH2 /
UDCH stage and the SACCH walk) between device events.  Two inputs, five distinct channels with different leads tiled to the batch, a
fresh stretch of the stream every call:

    cac     tests/nxdngen.cac_stream: a control channel, every frame a CAC (every slot wanted by the 175-step decoder)
    voice   the reference's NXDN96 capture (tests/golden/iq_nxdn96.npz) repeated: a voice call, no wanted slot

    python tools/bench_nxdn_ctrl_stage.py [--channels 1365] [--samples 48000] [--warmup 2] [--calls 8] [--ctrl 0|1] [--input cac|voice]

DDN_LIB_PATH names the library (a build of the parent commit reads the same input through these bindings; the entries it lacks are left
unbound).  Prints one line: median (min .. max) ms per call of the step and of stage 2, and what the stage saw."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DISTINCT = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1365)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--ctrl", type=int, default=0)
    ap.add_argument("--input", default="cac", choices=("cac", "voice"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "dsd-neo_amd", "bindings"), ROOT]
    import torch

    import ddn
    have = C.CDLL(ddn.LIB_PATH)
    for name in [k for k in ddn.PROTOTYPES if not hasattr(have, k)]:
        del ddn.PROTOTYPES[name]
    B, n = a.channels, a.samples
    assert B % DISTINCT == 0
    total = n * (a.warmup + a.calls)
    if a.input == "cac":
        import nxdngen
        import p25gen
        dib = nxdngen.cac_stream(total // 1920 + 4)
        src = np.stack([p25gen.modulate_cu8(dib, total, lead=300 + 531 * c, seed=4 + c) for c in range(DISTINCT)])
    else:
        iq = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "iq_nxdn96.npz"))["iq"], np.uint8)
        rep = np.tile(iq, (total // len(iq) + 2, 1))
        src = np.stack([rep[977 * c:977 * c + total] for c in range(DISTINCT)])
    src = torch.from_numpy(src).cuda()
    reps = B // DISTINCT
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_NXDN96, rf_mod=2, handlers=1, vocoder=0)
    if a.ctrl:
        ch.set_nxdn_ctrl(1)
    l = ddn.lib()
    st = torch.cuda.current_stream().cuda_stream
    step, dec, frames, wanted, good = [], [], 0, 0, 0
    for k in range(a.warmup + a.calls):
        x = src[:, k * n:(k + 1) * n].repeat(reps, 1, 1).contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        for stage in (0, 1):
            assert l.ddn_fsk4_chain_stage(ch.h, stage, x.data_ptr(), st) == 0
        ev[1].record()
        assert l.ddn_fsk4_chain_stage(ch.h, 2, x.data_ptr(), st) == 0
        ev[2].record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            step.append(ev[0].elapsed_time(ev[2]))
            dec.append(ev[1].elapsed_time(ev[2]))
            r = ch.results()
            S = int(r.max_syncs)
            frames += int(ch.fetch(r.d_valid, np.uint8, (B, S)).sum())
            if a.ctrl:
                f = ch.nxdn_ctrl_results().frames
                kind, ok = ch.fetch(f.d_kind, np.uint8, (B, S)), ch.fetch(f.d_crc_ok, np.uint8, (B, S))
                wanted += int((kind != 0).sum())
                good += int(((kind != 0) & (ok == 1)).sum())
    ch.close()
    step, dec = np.array(step), np.array(dec)
    print("%-12s step %.3f (%.3f .. %.3f)  stage 2 %.3f (%.3f .. %.3f) ms per call, %d calls; whole frames per call %.0f, control frames %.0f, "
          "CRC good %.0f" % (a.label or ("ctrl=%d" % a.ctrl), float(np.median(step)), step.min(), step.max(), float(np.median(dec)), dec.min(),
                             dec.max(), len(step), frames / len(step), wanted / len(step), good / len(step)), flush=True)


if __name__ == "__main__":
    main()
