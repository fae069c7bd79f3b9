"""What assembling DMR data PDUs on the device costs: stage 2 of the DMR chain (ddn_fsk4_chain_stage(c, 2, ...): frame FEC, data
bursts, and - once ddn_fsk4_chain_set_dmr_pdu_slots has been called - the marks and the PDU walk) between two device events, stages 0
and 1 queued in front of the first.  The input is tests/chain_fsk4_stream.dmr_data_stream traffic (every data type, both time slots),
five distinct channels with different leads tiled to the batch, a fresh stretch of the stream every call.

    python tools/bench_dmr_pdu_stage.py [--channels 1365] [--samples 48000] [--warmup 4] [--calls 24] [--pdu 0|1..8] [--traffic data|pdu] [--bindings DIR]

--bindings: the directory ddn.py is taken from (its library beside it): a build of another commit reads the same input.  Prints one
line: median (min .. max) ms per call of the timed calls, and what the walk saw."""
import argparse
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
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--pdu", type=int, default=0)
    ap.add_argument("--bindings", default=os.path.join(ROOT, "dsd-neo_amd", "bindings"))
    ap.add_argument("--label", default="")
    ap.add_argument("--traffic", default="data", choices=("data", "pdu"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.abspath(a.bindings), ROOT]
    import torch

    import chain_fsk4_stream as cs
    import ddn
    import p25gen
    B, n = a.channels, a.samples
    assert B % DISTINCT == 0
    total = n * (a.warmup + a.calls)
    rng = np.random.default_rng(11)
    if a.traffic == "pdu":              # whole PDUs of every kind (tests/dmrpdugen.air_plan) instead of single bursts
        import dmrpdugen
        dib = dmrpdugen.air_dibits(dmrpdugen.air_plan(0))
    else:
        dib = cs.dmr_data_stream(rng)[0]
    dib = np.tile(dib, total // (10 * len(dib)) + 2)
    src = torch.from_numpy(np.stack([p25gen.modulate_cu8(dib, total, lead=300 + 531 * c, seed=4 + c, noise=0.02) for c in range(DISTINCT)])).cuda()
    reps = B // DISTINCT
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=0)
    if a.pdu:
        ch.set_dmr_pdu_slots(a.pdu)
    l = ddn.lib()
    st = torch.cuda.current_stream().cuda_stream
    ms, bursts, pdus = [], 0, 0
    for k in range(a.warmup + a.calls):
        x = src[:, k * n:(k + 1) * n].repeat(reps, 1, 1).contiguous()
        for stage in (0, 1):
            assert l.ddn_fsk4_chain_stage(ch.h, stage, x.data_ptr(), st) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert l.ddn_fsk4_chain_stage(ch.h, 2, x.data_ptr(), st) == 0
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            ms.append(e0.elapsed_time(e1))
            bursts += int(ch.fetch(ch.results().d_dmr_n_data, np.int32, (B,)).sum())
            if a.pdu:
                pdus += int(ch.fetch(ch.dmr_pdu_results().out.d_n_pdus, np.int32, (B,)).sum())
    ch.close()
    ms = np.array(ms)
    print("%-10s %.3f (%.3f .. %.3f) ms per call, %d calls; data bursts per call %.0f, PDUs completed per call %.0f"
          % (a.label or ("pdu=%d" % a.pdu), float(np.median(ms)), ms.min(), ms.max(), len(ms), bursts / len(ms), pdus / len(ms)), flush=True)


if __name__ == "__main__":
    main()
