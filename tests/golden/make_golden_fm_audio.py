"""Generator of tests/golden/fm_audio_*.npz: small seeded cu8 / cs16 inputs and what the COMPILED REFERENCE's full_demod() gives for them
in the audio-monitor output kind (driver: tests/fm_audio_refdrv.cpp around oracle/_ref/libdsdneo_ref.so), with the carried state and the
decimator taps.  Run where the reference and oracle/_ref exist:  python tests/golden/make_golden_fm_audio.py
Each file: cfg_json, iq [2, n, 2], calls, audio [2, count] float32, state [2, 8] float32, taps [16] float32."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fm_audio  # noqa: E402


def main():
    assert fm_audio.have_reference(), "needs the reference's headers and oracle/_ref/libdsdneo_ref.so"
    for k, (name, over) in enumerate(fm_audio.GOLDEN.items()):
        c = fm_audio.cfg(**over)
        fmt = "cs16" if k % 2 else "cu8"
        iq = fm_audio.synth_nfm(900 + k, 2, fm_audio.GOLDEN_N, fmt=fmt, amp_blocks=fm_audio.GOLDEN_AMPS)
        rows, states, taps = [], [], np.zeros(16, np.float32)
        for ch in range(2):
            r = fm_audio.Reference(c)
            parts, pos = [], 0
            for m in fm_audio.GOLDEN_CALLS:
                parts.append(r.run(iq[ch, pos:pos + m]))
                pos += m
            rows.append(np.concatenate(parts))
            states.append(r.state())
            t = r.taps()
            taps = t if t is not None else taps
            r.close()
        np.savez_compressed(fm_audio.golden_path(name), cfg_json=json.dumps(c), iq=iq, calls=np.array(fm_audio.GOLDEN_CALLS, np.int32),
                            audio=np.stack(rows), state=np.stack(states), taps=taps)
        print(name, fmt, np.stack(rows).shape, os.path.getsize(fm_audio.golden_path(name)))


if __name__ == "__main__":
    main()
