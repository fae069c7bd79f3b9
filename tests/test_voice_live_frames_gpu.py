"""The chain object's voice stage works on the live slots of a call only: the slots that hold a frame are bit-exact
against the whole-stream oracle, and every slot that holds none keeps, in every array ddn_p25_chain_get_results hands out, the bytes
the whole-array kernels used to leave there - the dead pattern, which this test takes from the public batch entry points (one
all-zero IMBE frame with its skip flag), not from the chain.

Five channels, three calls of 2.3 LDUs' worth of samples + the flush, max_ldu = 3 (27 voice slots per channel):
  0  voice from the start: one LDU in call 1, two in call 2 - a live prefix and a dead tail
  1  control channel: never a voice frame
  2  one LDU in call 1, nothing after it: its slots go from live to dead (the pattern has to come back)
  3  nothing in call 1, one LDU in call 2 and another in call 3: dead to live, and the vocoder's carried state across the gap
  4  three LDUs in call 2: as many as max_ldu, no dead slot
and nothing on any channel in the flush: an empty live list."""
import ctypes as C

import numpy as np
import pytest

import chain_stream
import ddn
import mbe
import p25gen

pytestmark = pytest.mark.gpu

B, N_CALL, CALLS, MAX_LDU, NAC = 5, 20000, 3, 3, 0x293


def _burst(rng, n):
    """a header unit (the first NID of a transmission is read while the slicer settles and may fail) + n LDUs"""
    ldus = p25gen.make_ldus(rng, n, NAC, np.stack([mbe.imbe_encode(b) for b in mbe.random_imbe_bits(rng, (9 * n,))]))[0]
    return np.concatenate([p25gen.make_hdu(rng, NAC)[0], ldus])


@pytest.fixture(scope="module")
def traffic(built):
    """(iq u8 [B][n_total][2], the oracle's whole-stream answer per channel) - computed once, read by both ways of running"""
    rng = np.random.default_rng(20260)
    n_total = N_CALL * CALLS
    ctl = np.concatenate([p25gen.make_hdu(rng, NAC)[0]] + [p25gen.make_frames(rng, 1, NAC, crc=True, blocks=1 + k % 3)[0] for k in range(14)])
    first = _burst(rng, 1)
    dib = [_burst(rng, 3), ctl, _burst(rng, 1), np.concatenate([first, np.zeros(2000 - len(first), np.int8), _burst(rng, 1)]), _burst(rng, 3)]
    lead = [300, 337, 300, 11000, 7000]
    iq = np.stack([p25gen.modulate_cu8(dib[c], n_total, lead=lead[c], seed=c) for c in range(B)])
    want = [chain_stream.run_stream(iq[c], N_CALL, seed=c) for c in range(B)]
    return iq, want


@pytest.fixture(scope="module")
def dead(built):
    """what a slot without a frame holds: bits [88], result [5], PCM [160], result after synthesis [5]"""
    l = ddn.lib()
    sizes = dict(fr=184, fl=1, bits=88, res=20, pcm=640, res_out=20)
    p = {}
    for k, n in sizes.items():
        p[k] = C.c_void_p()
        assert l.ddn_device_alloc(n, C.byref(p[k])) == 0
    assert l.ddn_device_upload(p["fr"], np.zeros(184, np.uint8).ctypes.data, 184) == 0
    assert l.ddn_device_upload(p["fl"], np.full(1, 0xFF, np.uint8).ctypes.data, 1) == 0
    assert l.ddn_mbe_frame_decode_batch(ddn.MBE_IMBE, p["fr"], None, 1, p["bits"], p["res"], None) == 0
    assert l.ddn_mbe_result_skip_batch(p["fl"], 1, p["res"], None) == 0
    voc = C.c_void_p()
    assert l.ddn_mbe_batch_create(ddn.MBE_IMBE, 1, C.byref(voc)) == 0
    assert l.ddn_mbe_batch_set_p25p1_tail_rule(voc, 1) == 0
    assert l.ddn_mbe_synth_batch(voc, p["bits"], p["res"], 1, p["pcm"], p["res_out"], None) == 0
    out = {}
    for k, dt in (("bits", np.uint8), ("res", np.int32), ("pcm", np.float32), ("res_out", np.int32)):
        out[k] = np.zeros(sizes[k] // np.dtype(dt).itemsize, dt)
        assert l.ddn_device_download(out[k].ctypes.data, p[k], sizes[k]) == 0
    l.ddn_mbe_batch_destroy(voc)
    for q in p.values():
        l.ddn_device_free(q)
    assert out["res"][0] < 0 and not out["pcm"].any()      # the skip flag is the result's top bit; a skipped frame is silent
    return out


def _run(iq, how, dead):
    """three calls + the flush; after each, every slot behind a channel's LDUs is compared with the dead pattern -> (Collector,
    n_ldu per call [CALLS + 1][B])"""
    ch = ddn.P25ChainC(B, N_CALL, max_ldu=MAX_LDU)
    assert ch.Fv == MAX_LDU
    col = chain_stream.Collector(ch)
    slots = MAX_LDU * 9
    n_ldu = []

    def look(call):
        col.take()
        r = ch.results()
        k = ch.fetch(r.d_n_ldu, np.int32, (B,))
        n_ldu.append(k)
        got = dict(bits=ch.fetch(r.d_imbe_bits, np.uint8, (B, slots, 88)), res=ch.fetch(r.d_imbe_result, np.int32, (B, slots, 5)),
                   pcm=ch.fetch(r.d_pcm, np.float32, (B, slots, 160)), res_out=ch.fetch(r.d_synth_result, np.int32, (B, slots, 5)))
        for c in range(B):
            for name, a in got.items():
                tail = a[c, 9 * k[c]:]
                assert np.array_equal(tail.view(np.uint8), np.broadcast_to(dead[name], tail.shape).view(np.uint8)), (how, call, c, name)

    for k in range(CALLS):
        part = np.ascontiguousarray(iq[:, k * N_CALL:(k + 1) * N_CALL])
        d = C.c_void_p()
        assert ddn.lib().ddn_device_alloc(part.nbytes, C.byref(d)) == 0
        assert ddn.lib().ddn_device_upload(d, part.ctypes.data, part.nbytes) == 0
        if how == "run":
            ch.run(d)
        else:
            ch.run_pipelined(d)
            ch.wait()
        ddn.lib().ddn_device_free(d)
        look(k)
    ch.flush()
    look(CALLS)
    ch.close()
    return col, np.stack(n_ldu)


@pytest.mark.parametrize("how", ["run", "run_pipelined"])
def test_live_slots_match_the_oracle_and_dead_slots_keep_their_pattern(traffic, dead, how):
    iq, want = traffic
    col, n_ldu = _run(iq, how, dead)
    # the traffic is what the docstring says it is (a shape that drifts would leave a path of the kernels untested)
    assert 0 < n_ldu[0, 0] < MAX_LDU and (n_ldu[:, 0] > 0).sum() >= 2, n_ldu
    assert not n_ldu[:, 1].any(), n_ldu
    assert n_ldu[0, 2] == 1 and not n_ldu[1:, 2].any(), n_ldu
    assert n_ldu[0, 3] == 0 and n_ldu[1, 3] == 1 and n_ldu[2, 3] == 1, n_ldu
    assert n_ldu[1, 4] == MAX_LDU, n_ldu
    assert not n_ldu[CALLS].any(), n_ldu
    # live slots: voice bits, result words and PCM of every frame, in order, against the whole-stream oracle - which carries the
    # vocoder's state of channel 3 from its first burst across the empty slots into its second
    voiced = 0
    for c in range(B):
        voiced += chain_stream.check_channel(col, c, want[c])[2]
    assert voiced == 9 * int(n_ldu.sum()) == 9 * 9, (voiced, n_ldu)
    assert len(col.voice[3]) == 18 and np.abs(np.concatenate([v[4] for v in col.voice[3][9:]])).sum() > 0
