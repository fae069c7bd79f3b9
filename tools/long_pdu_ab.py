"""What the long data unit switch (ddn_p25_chain_set_long_data_units) costs: the P25 chain at 4096 channels x 48000 samples, one
stream (ddn_p25_chain_run), in four cases - traffic without data units (voice + TSDUs) with the switch off and on; every channel
carrying back-to-back 20-block units with the switch off and on (the receive loop's time differs with the traffic: the switch's
cost is the difference within a traffic pair).  Per case: the step (events around `steps` back-to-back calls) and the decode stage
(ddn_p25_chain_get_stage_ms [2]: framer + frame FEC + data units, stage timing on, mean over `steps` calls).  The input is eight
distinct channels tiled to the batch, a fresh stretch of the stream every call.

    python tools/long_pdu_ab.py [--channels 4096] [--samples 48000] [--steps 8] [--out profiles/long_pdu_ab.txt]"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "dsd-neo_amd", "bindings"), ROOT]

import ddn  # noqa: E402
import mbe  # noqa: E402
import p25gen  # noqa: E402

NAC = 0x293
DISTINCT = 8


def traffic(kind, n_total, seed):
    rng = np.random.default_rng(seed)
    parts = [p25gen.make_frames(rng, 1, NAC, crc=True, blocks=1)[0], np.zeros(160, np.int8)]
    while sum(len(p) for p in parts) * 10 < n_total:
        if kind == "pdu":
            parts.append(p25gen.make_pdu_coded(rng, NAC, blks=20)[0])
        elif rng.random() < 0.5:
            bits = mbe.random_imbe_bits(rng, (18,))
            parts.append(p25gen.make_ldus(rng, 2, NAC, np.stack([mbe.imbe_encode(b) for b in bits]))[0])
        else:
            parts.append(p25gen.make_frames(rng, 2, NAC, crc=True, blocks=3)[0])
    return p25gen.modulate_cu8(np.concatenate(parts), n_total, lead=200 + 37 * seed, seed=seed, noise=0.03)


def measure(torch, B, n, steps, kind, switch):
    calls = 3 + steps + 3 + steps
    src = torch.from_numpy(np.stack([traffic(kind, n * calls, s) for s in range(DISTINCT)])).cuda()   # [8][n calls][2]
    reps = B // DISTINCT

    def call(k):
        return src[:, k * n:(k + 1) * n].repeat(reps, 1, 1).contiguous()

    ch = ddn.P25ChainC(B, n)
    if switch:
        ch.set_long_data_units(127, 0)
    stream = torch.cuda.current_stream()
    k = 0
    for _ in range(3):
        ch.run(call(k).data_ptr(), stream.cuda_stream)
        k += 1
    xs = [call(k + i) for i in range(steps)]
    k += steps
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for x in xs:
        ch.run(x.data_ptr(), stream.cuda_stream)
    e1.record()
    torch.cuda.synchronize()
    step = e0.elapsed_time(e1) / steps
    del xs
    ch.set_timing(1)
    dec = []
    for i in range(3 + steps):
        x = call(k)
        k += 1
        ch.run(x.data_ptr(), stream.cuda_stream)
        t = ch.stage_ms()
        if i >= 3:
            dec.append(float(t[2]))
    units = 0
    if switch:
        r = ch.long_pdu_results()
        units = int(ch.fetch(r.d_n, np.int32, (B,)).sum())
    ch.close()
    return step, float(np.mean(dec)), float(np.min(dec)), units


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert a.channels % DISTINCT == 0
    lines = ["long data units, A/B: P25 chain %d channels x %d samples, ddn_p25_chain_run on one stream, %d steps per case"
             % (a.channels, a.samples, a.steps),
             "%-44s %10s %16s %16s %8s" % ("case", "step ms", "decode ms mean", "decode ms min", "units")]
    for name, kind, switch in (("no data units, switch off", "voice", False), ("no data units, switch on", "voice", True),
                               ("back-to-back 20-block units, switch off", "pdu", False),
                               ("back-to-back 20-block units, switch on", "pdu", True)):
        step, dmean, dmin, units = measure(torch, a.channels, a.samples, a.steps, kind, switch)
        lines.append("%-44s %10.3f %16.3f %16.3f %8s" % (name, step, dmean, dmin, units if switch else "-"))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
