"""What decoding DMR MS / direct-mode bursts on the device costs: a DMR chain's whole step (ddn_fsk4_chain_stage 0, 1, 2) and its stage 2
alone (burst gather, the BS data / embedded-signalling / voice stages and - once ddn_fsk4_chain_set_dmr_ms has been called - the MS
walk, gathers, FEC and vocoder) between device events.  Two inputs, five distinct channels with different leads tiled to the batch, a
fresh stretch of the stream every call:

    voice   tests/dmrmsgen voice units back to back behind the MS voice word (a burst every 288 symbols, a link control per unit)
    data    data bursts behind the MS data word, one every 288 symbols: CSBKs, full link control, rate 3/4 (every fourth burst)

    python tools/bench_dmr_ms_stage.py [--channels 1365] [--samples 48000] [--warmup 2] [--calls 8] [--ms 0|1] [--input voice|data]

DDN_LIB_PATH names the library (a build of the parent commit reads the same input through these bindings; the entries it lacks are left
unbound).  With --ms 0 the loop holds its default counts behind the MS words, as the parent does.  Prints one line: median (min .. max)
ms per call of the step and of stage 2, and what the stage listed."""
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
    ap.add_argument("--ms", type=int, default=0)
    ap.add_argument("--vocoder", type=int, default=1)
    ap.add_argument("--input", default="voice", choices=("voice", "data"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "dsd-neo_amd", "bindings"), ROOT]
    import torch

    import ddn
    have = C.CDLL(ddn.LIB_PATH)
    for name in [k for k in ddn.PROTOTYPES if not hasattr(have, k)]:
        del ddn.PROTOTYPES[name]
    import dmrmsgen as gen
    import p25gen
    B, n = a.channels, a.samples
    assert B % DISTINCT == 0
    total = n * (a.warmup + a.calls)
    rng = np.random.default_rng(11)
    bursts = []
    while 288 * len(bursts) * 10 < total + 6000:
        if a.input == "voice":
            bursts += gen.voice_unit(3, 7, rng.integers(0, 2, 72).astype(np.uint8), rng)
        else:
            ty = (3, 1, 6, 8)[len(bursts) % 4]
            bursts.append(gen.burst(2, 7, ty, gen.data_info(ty, rng), rng))
    dib = gen.air(bursts, rng)
    src = np.stack([p25gen.modulate_cu8(dib, total, lead=300 + 531 * c, seed=4 + c) for c in range(DISTINCT)])
    src = torch.from_numpy(src).cuda()
    reps = B // DISTINCT
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=a.vocoder)
    if a.ms:
        ch.set_dmr_ms(1)
    l = ddn.lib()
    st = torch.cuda.current_stream().cuda_stream
    step, dec, syncs, listed = [], [], 0, np.zeros(3, np.int64)
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
            syncs += int(ch.fetch(ch.results().d_n_sync, np.int32, (B,)).sum())
            if a.ms:
                b = ch.dmr_ms_results().bursts
                listed += [int(ch.fetch(p, np.int32, (B,)).sum()) for p in (b.d_n_data, b.d_n_voice, b.d_n_lc)]
    if a.ms:
        assert not ch.fetch(ch.dmr_ms_results().bursts.d_dropped, np.int32, (B,)).any()
    ch.close()
    step, dec = np.array(step), np.array(dec)
    print("%-12s step %.3f (%.3f .. %.3f)  stage 2 %.3f (%.3f .. %.3f) ms per call, %d calls; per call: syncs %.0f, data bursts %.0f, voice "
          "bursts %.0f, link controls %.0f" % (a.label or ("ms=%d" % a.ms), float(np.median(step)), step.min(), step.max(), float(np.median(dec)),
                                               dec.min(), dec.max(), len(step), syncs / len(step), *(listed / len(step))), flush=True)


if __name__ == "__main__":
    main()
