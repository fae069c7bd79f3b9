"""The receive loop's lean runs at the headline shape (4096 channels x 48 000 cu8 samples, handlers inside the loop, the kernel
instance bench.py times) against the whole-stream CPU oracle (tests/chain_stream.py): two calls of a stream + the flush, dibit
records, flags, the handlers' decisions, NIDs, TSDU blocks and voice bit-exact - on voice-only, control-only and mixed traffic,
and on channels whose frames end at every sample offset of a 128-sample tile (the run length's tile, lock and handler-phase
limits all meet there)."""
import os
import sys

import numpy as np
import pytest
import torch

import chain_stream
import ddn
import p25gen

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (the headline traffic)

pytestmark = pytest.mark.gpu

B, N = 4096, 48000


@pytest.fixture(scope="module")
def base_traffic():
    return bench.make_base_traffic(N)


def _run_and_check(iq, pick):
    """iq u8 [B][n][2] replayed as two calls + the flush through the chain object; `pick`: the channels compared"""
    Bc, n = iq.shape[0], iq.shape[1]
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
    ch = ddn.P25ChainC(Bc, n, block_len=8192)
    try:
        col = chain_stream.Collector(ch, channels=pick)
        for _ in range(2):
            ch.run_pipelined(d_iq.data_ptr())
            ch.wait()
            col.take()
        ch.flush()
        col.take()
        tot = np.zeros(3, np.int64)
        for i, c in enumerate(pick):
            want = chain_stream.run_stream(np.concatenate([iq[c], iq[c]]), n, seed=c)
            tot += chain_stream.check_channel(col, i, want)
        return tot
    finally:
        ch.close()


def _pick(Bc, k):
    """k channels spread over the batch, the first and last workgroups and both recurrence waves of a workgroup among them"""
    return sorted(set(int(c) for c in [0, 1, 2, 3, 4, 5, 6, 7, Bc - 8, Bc - 5, Bc - 1] + list(np.linspace(0, Bc - 1, k).astype(int))))


@pytest.mark.parametrize("kind", ["voice", "ctrl", "mixed"])
def test_lean_runs_headline_shape(base_traffic, kind):
    voice, ctrl = base_traffic
    src = []
    for c in range(B):
        k, bi = bench.channel_source(c)
        if kind != "mixed":
            k = kind
        src.append((voice if k == "voice" else ctrl)[bi])
    iq = np.stack(src)
    tot = _run_and_check(iq, _pick(B, 48))
    if kind != "ctrl":
        assert tot[2] > 0, tot
    if kind != "voice":
        assert tot[1] > 0, tot
    assert tot[0] > 0, tot


@pytest.mark.parametrize("kind", ["voice", "ctrl"])
def test_lean_runs_frame_ends_at_tile_edges(kind):
    """128 channels whose traffic starts one sample later each: every frame end (and so every end of a lock or of a phase that
    ends in a handler's decision) lands on every sample offset of the 128-sample tile in one channel or another"""
    import mbe
    n = 12800
    rng = np.random.default_rng(77 if kind == "voice" else 78)
    if kind == "voice":
        frames = np.stack([mbe.imbe_encode(b) for b in mbe.random_imbe_bits(rng, (18,))])
        dib = np.concatenate([p25gen.make_hdu(rng, 0x293)[0], p25gen.make_ldus(rng, 2, 0x293, frames)[0],
                              p25gen.make_tdulc(rng, 0x293)[0], p25gen.make_tdu(0x293)])
    else:
        dib = np.concatenate([p25gen.make_frames(rng, 1, 0x293, crc=True, blocks=1 + k % 3)[0] for k in range(12)])
    Bc = 128
    iq = np.stack([p25gen.modulate_cu8(dib, 2 * n, lead=300 + c, seed=c)[:n] for c in range(Bc)])
    tot = _run_and_check(iq, list(range(Bc)))
    assert tot[0] > 0, tot
