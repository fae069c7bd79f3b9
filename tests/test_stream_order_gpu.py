"""GPU: the stream-taking entry points of the C ABI keep stream order on a stream that is not the null stream.  Every call runs
behind the late producer of tests/stream_order.py: its inputs arrive on the stream after a delay, its outputs are copied away and
overwritten on the stream right behind it, and it has returned to the host before the delay ends.  What it computes must equal the
reference the existing tests pin (the `_host` variant, the CPU oracle, or the same object driven on the null stream with a device
synchronisation after every call).  Two data sets on two streams, issued with no host wait between them, must each equal their own
reference: nothing is shared between calls on different streams.

The CPU test at the end (not marked gpu) keeps the module complete: every prototype of include/*.h with a stream parameter is driven
here (DRIVEN) or reached through a driven call that passes its own stream on (REACHED_ON_STREAM); a new stream-taking export fails
the test until it is one of the two."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddn
import stream_order as so
from test_host_staging_gpu import BATCH_ONLY_NULL, CALLS, F32, _base, _is_ptr

gpu = pytest.mark.gpu

DRIVEN = set()      # the stream-taking exports the cases below call with the late producer's stream


# ---- the harness has teeth ---------------------------------------------------------------------------------------------------------------
@gpu
def test_a_call_on_the_wrong_stream_is_detected(built):
    """a stateless call issued on the NULL stream while the producer sits on `s` reads the decoy (valid data nothing is writing at
    the time) and gives the decoy's result, which differs from the true one: the misordered call shows"""
    import torch
    l = ddn.lib()
    n = 64
    rng = np.random.default_rng(5)
    truth, decoy = rng.integers(0, 2, (n, 10)).astype(np.uint8), rng.integers(0, 2, (n, 10)).astype(np.uint8)
    want = {}
    for key, v in (("truth", truth), ("decoy", decoy)):
        w, ok = v.copy(), np.zeros(n, np.uint8)
        assert l.ddn_fec_hamming_10_6_3_host(w.ctypes.data, n, ok.ctypes.data) == 0
        want[key] = w.tobytes() + ok.tobytes()
    assert want["truth"] != want["decoy"]
    p = so.Late()
    bits, ok = p.inout(truth, decoy), p.output(n)
    p.begin()
    assert l.ddn_fec_hamming_10_6_3_batch(bits.data_ptr(), n, ok.data_ptr(), None) == 0       # the null stream: not ordered behind s
    torch.cuda.current_stream().synchronize()
    got = bits.cpu().numpy().tobytes() + ok.cpu().numpy().tobytes()
    p.finish("wrong-stream self-test")
    p.wait()
    assert got == want["decoy"] and got != want["truth"]


@gpu
def test_the_stream_does_not_wait_for_the_null_stream(built):
    import torch
    s = so.new_stream()
    assert so.stream_flags(s.cuda_stream) & so.HIP_STREAM_NON_BLOCKING
    torch.cuda._sleep(so.delay_cycles())                 # the null stream is busy ...
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        x = torch.zeros(16, device="cuda")
        done.record(s)
    done.synchronize()                                   # ... and work on `s` ends before it
    assert not ev.query()
    torch.cuda.synchronize()
    del x


# ---- the stateless calls with a `_host` twin -----------------------------------------------------------------------------------------------
def _draw(name, seed):
    """the arguments of CALLS[name] drawn as tests/test_host_staging_gpu.py draws them -> [(spec, value or None)]"""
    rng = np.random.default_rng(seed)
    vals = []
    for a in CALLS[name]:
        if not _is_ptr(a) or isinstance(a, np.ndarray):
            vals.append((a, None))
            continue
        role, dtype, count, lo, hi = a
        if isinstance(lo, np.ndarray):
            v = lo.astype(dtype)
        else:
            v = (rng.normal(0, hi, count) if dtype == F32 else rng.integers(lo, hi, count)).astype(dtype)
        if _base(role) == "out":
            v = np.zeros(count, dtype)
        vals.append((a, v))
    return vals


def _host_reference(name, vals):
    """the `_host` variant on copies -> {argument index: bytes} of every output"""
    l = ddn.lib()
    args, outs, alive = [], {}, []                       # alive: every copy stays until the call is through
    for k, (a, v) in enumerate(vals):
        if a is BATCH_ONLY_NULL:
            continue
        if isinstance(a, np.ndarray):
            args.append(a.ctypes.data)
        elif v is None:
            args.append(a)
        else:
            w = v.copy()
            alive.append(w)
            args.append(w.ctypes.data)
            if _base(a[0]) in ("out", "io"):
                outs[k] = w
    assert getattr(l, name)(*args) == 0, l.ddn_last_error()
    return {k: w.tobytes() for k, w in outs.items()}


def _batch_args(vals, buf, stream):
    args = []
    for k, (a, v) in enumerate(vals):
        if a is BATCH_ONLY_NULL:
            args.append(None)
        elif isinstance(a, np.ndarray):
            args.append(a.ctypes.data)
        elif v is None:
            args.append(a)
        else:
            args.append(buf[k].data_ptr())
    return args + [stream]


def _unwritten(name, vals):
    """the output bytes the call leaves alone, from a warm-up call on the null stream with a device synchronisation behind it: a
    byte that still holds the marker where the `_host` variant (whose staging zero-fills its outputs) gives zero.  The warm-up also
    takes first-use costs out of the calls that must return within the delay."""
    import torch
    l = ddn.lib()
    buf = {}
    for k, (a, v) in enumerate(vals):
        if v is not None:
            buf[k] = torch.from_numpy(v.view(np.uint8).copy()).cuda()
            if _base(a[0]) == "out":
                buf[k].fill_(so.MARKER)
    torch.cuda.synchronize()
    assert getattr(l, name[:-5] + "_batch")(*_batch_args(vals, buf, None)) == 0, l.ddn_last_error()
    torch.cuda.synchronize()
    ref = _host_reference(name, vals)
    left = {}
    for k, h in ref.items():
        g, h = buf[k].cpu().numpy(), np.frombuffer(h, np.uint8)
        left[k] = (g == so.MARKER) & (h == 0) if _base(vals[k][0][0]) == "out" else np.zeros(len(h), bool)
        assert np.array_equal(np.where(left[k], 0, g), h), (name, k)
    return ref, left


class _Case:
    """one data set of one stateless call behind its own late producer"""

    def __init__(self, name, seed):
        self.name, self.batch = name, name[:-5] + "_batch"
        self.vals, decoy = _draw(name, seed), _draw(name, seed + 500)
        self.ref, self.left = _unwritten(name, self.vals)
        self.decoy_ref = _host_reference(name, decoy)
        self.p = so.Late()
        self.buf = {}
        for k, ((a, v), (_, d)) in enumerate(zip(self.vals, decoy)):
            if v is None:
                continue
            role = _base(a[0])
            self.buf[k] = self.p.output(v.nbytes) if role == "out" else (self.p.inout(v, d) if role == "io" else self.p.input(v, d))

    def issue(self):
        l = ddn.lib()
        assert getattr(l, self.batch)(*_batch_args(self.vals, self.buf, self.p.handle)) == 0, l.ddn_last_error()

    def check(self):
        assert self.ref
        for k, h in self.ref.items():
            want = np.where(self.left[k], so.MARKER, np.frombuffer(h, np.uint8))
            got = self.p.kept(self.buf[k])
            assert np.array_equal(got, want), (self.name, k, np.flatnonzero(got != want)[:8])


# calls whose result is the same for every random input (random words fail their check sums alike): the decoy's result cannot be
# told from the true one, so only a write on the wrong stream would show in them
SAME_RESULT_ON_RANDOM_INPUT = {"ddn_fec_isch_lookup_host", "ddn_fec_p25_crc16_host", "ddn_p25p2_mac_crc_host", "ddn_p25p2_sync_cut_host"}


@gpu
@pytest.mark.parametrize("name", sorted(CALLS))
def test_stateless_call_behind_a_late_producer(built, name):
    c = _Case(name, 100 + sorted(CALLS).index(name))
    if name not in SAME_RESULT_ON_RANDOM_INPUT:
        assert c.decoy_ref != c.ref, "the decoy's result equals the true one"
    c.p.begin()
    c.issue()
    c.p.finish(c.batch)
    c.p.wait()
    c.check()


@gpu
@pytest.mark.parametrize("name", sorted(CALLS))
def test_stateless_call_on_two_streams_at_once(built, name):
    import torch
    a, b = _Case(name, 200 + sorted(CALLS).index(name)), _Case(name, 300 + sorted(CALLS).index(name))
    if name not in SAME_RESULT_ON_RANDOM_INPUT:
        assert a.ref != b.ref
    so.delay_cycles()
    torch.cuda.synchronize()
    a.p.begin(settle=False)
    b.p.begin(settle=False)
    a.issue()
    b.issue()
    a.p.finish(a.batch)
    b.p.finish(b.batch)
    a.p.wait()
    b.p.wait()
    a.check()
    b.check()


DRIVEN.update(n[:-5] + "_batch" for n in CALLS)


# ---- the stateful stage objects ------------------------------------------------------------------------------------------------------------
# One scheme for every object: a case is a list of operations, ("run", n, [input arrays]) or ("reset",).  _solo() is the reference
# run: a fresh object, the null stream, a device synchronisation after every operation, outputs that start as marker bytes.  The same
# operations behind a late producer must leave the same bytes in every output buffer and the same readable state.  Where the CPU
# oracle of the object is at hand (Stage.oracle) the solo run is held against it as well, so that the reference of the comparison is
# the oracle's and not the device's own.
B5 = 5              # a partial wavefront


class Stage:
    """what the scheme needs to know of one object; `lens` = (the shorter first call, the longer second call)"""
    name = None         # the run call
    reset_name = None   # the reset that takes a stream, if the object has one
    lens = (0, 0)
    grows = False       # a longer call replaces a buffer of the object (and waits for the stream first: stream_order.GROWS_ON_HOST)

    def make(self):
        raise NotImplementedError

    def gen(self, seed, k, n):
        """-> the input arrays of call k (of length n) of the input stream `seed`"""
        raise NotImplementedError

    def plan(self, obj, n):
        """-> the size in bytes of every output buffer of a call of length n"""
        raise NotImplementedError

    def launch(self, obj, ins, n, outs, stream):
        raise NotImplementedError

    def reset(self, obj, stream):
        raise NotImplementedError

    def state(self, obj):
        """the readable carried state (synchronous getters) -> bytes"""
        return b""

    def oracle(self, runs, outs):
        """runs: the ("run", n, xs) operations of one fresh object in order, outs: their output buffers as uint8 arrays"""

    def oracle_after_reset(self, runs, outs):
        self.oracle(runs, outs)

    def forget(self, obj):
        """drop what the host side of the scheme noted of the calls so far (the counts a call returned, the lengths it was given)"""
        for k in ("counts", "lens"):
            if hasattr(obj, k):
                setattr(obj, k, [])

    def close(self, obj):
        if hasattr(obj, "close"):
            obj.close()


def _f32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class FrontEnd(Stage):
    name, reset_name, lens, blk = "ddn_front_end_run", "ddn_batch_reset", (2800, 4000), 1200

    def make(self):
        return ddn.Batch(B5, block_len=self.blk)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import orc
        return [orc.synth_c4fm_cu8(seed, B5, n, sps=10)]

    def plan(self, obj, n):
        return [B5 * n * 4]

    def launch(self, obj, ins, n, outs, stream):
        obj.run_device(ins[0], n, outs[0], stream)

    def reset(self, obj, stream):
        obj.reset(stream)

    def state(self, obj):
        return b"".join(obj.fsk_state(c).tobytes() for c in range(B5))

    def oracle(self, runs, outs):
        import orc
        fes = [orc.OracleFrontEnd() for _ in range(B5)]
        for (_, n, xs), o in zip(runs, outs):
            got = o[0].view(np.float32).reshape(B5, n)
            for c in range(B5):
                assert np.array_equal(_f32(got[c]), _f32(fes[c].run_cu8(xs[0][c], self.blk))), (self.name, c)


class FrontEndHalfband(FrontEnd):
    """one decimation pass in front: the cascade's buffer grows with the call"""
    grows = True

    def make(self):
        b = ddn.Batch(B5, block_len=self.blk)
        b.set_decimation(1)
        return b

    def gen(self, seed, k, n):
        import orc
        return [orc.synth_c4fm_cu8(seed + 17 * k, B5, n, sps=20)]

    def plan(self, obj, n):
        return [B5 * (n >> 1) * 4]

    def oracle(self, runs, outs):
        import orc
        fes = [orc.OracleFrontEnd(downsample_passes=1) for _ in range(B5)]
        for (_, n, xs), o in zip(runs, outs):
            got = o[0].view(np.float32).reshape(B5, n >> 1)
            for c in range(B5):
                assert np.array_equal(_f32(got[c]), _f32(fes[c].run_cu8(xs[0][c], self.blk))), (self.name, c)


class FrontEndSegments(FrontEnd):
    name, counts = "ddn_front_end_run_segments", (2, 3)

    def make(self):
        b = ddn.Batch(B5, lpf_profile=ddn.LPF_P25_C4FM, block_len=self.blk)
        cnt, prof = np.array(self.counts, np.int32), np.array([ddn.LPF_P25_C4FM, ddn.LPF_12K5], np.int32)
        assert ddn.lib().ddn_batch_set_segments(b.h, 2, cnt.ctypes.data, prof.ctypes.data) == 0
        return b

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import orc
        return [orc.synth_c4fm_cu8(seed + 31 * j, c, n, sps=10) for j, c in enumerate(self.counts)]

    def plan(self, obj, n):
        return [c * n * 4 for c in self.counts]

    def launch(self, obj, ins, n, outs, stream):
        ia, oa = (C.c_void_p * 2)(*ins), (C.c_void_p * 2)(*outs)
        assert ddn.lib().ddn_front_end_run_segments(obj.h, ia, n, oa, stream) == 0, ddn.lib().ddn_last_error()

    def oracle(self, runs, outs):
        import orc
        fes = [[orc.OracleFrontEnd(profile=p) for _ in range(c)] for p, c in zip((ddn.LPF_P25_C4FM, ddn.LPF_12K5), self.counts)]
        for (_, n, xs), o in zip(runs, outs):
            for j, c in enumerate(self.counts):
                got = o[j].view(np.float32).reshape(c, n)
                for ch in range(c):
                    assert np.array_equal(_f32(got[ch]), _f32(fes[j][ch].run_cu8(xs[j][ch], self.blk))), (self.name, j, ch)


class FmAudioStage(Stage):
    name, reset_name, lens, blk, grows = "ddn_fm_audio_run", "ddn_batch_reset", (1024, 1800), 256, True

    def cfg(self):
        import fm_audio
        return fm_audio.cfg(M=3)

    def make(self):
        import fm_audio
        return fm_audio.make_batch(ddn, self.cfg(), B5, ddn.IN_CU8, block_len=self.blk)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import fm_audio
        return [fm_audio.synth_nfm(seed, B5, n, block_len=self.blk)]

    def plan(self, obj, n):
        return [B5 * max(1, obj.max_samples(n)) * 4]

    def launch(self, obj, ins, n, outs, stream):
        obj.counts = getattr(obj, "counts", []) + [obj.run_device(ins[0], n, outs[0], max(1, obj.max_samples(n)), stream)]

    def reset(self, obj, stream):
        obj.reset(stream)

    def state(self, obj):
        return b"".join(obj.audio_state(c).tobytes() for c in range(B5)) + repr(obj.counts).encode()

    def oracle(self, runs, outs):
        import fm_audio
        rs = [fm_audio.Restatement(self.cfg(), self.blk) for _ in range(B5)]
        for (_, n, xs), o in zip(runs, outs):
            got = o[0].view(np.float32).reshape(B5, -1)
            for c in range(B5):
                want = rs[c].run(xs[0][c])
                assert len(want) > 0 and np.array_equal(_f32(got[c, :len(want)]), _f32(want)), (self.name, c)


class P25RxStage(Stage):
    name, lens, grows = "ddn_p25_rx_run", (3000, 6000), True

    def make(self):
        return ddn.P25Rx(B5, lock_symbols=408, use_matched_filter=1)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import orc
        return [orc.synth_p25_disc(seed, B5, n, frame_dibits=432)[0]]

    def plan(self, obj, n):
        ms = ddn.lib().ddn_p25_rx_max_symbols(obj.h, n)
        return [B5 * ms * 10, B5 * ms, B5 * 4]

    def launch(self, obj, ins, n, outs, stream):
        l = ddn.lib()
        assert l.ddn_p25_rx_run(obj.h, ins[0], n, outs[0], outs[1], outs[2], l.ddn_p25_rx_max_symbols(obj.h, n), stream) == 0, l.ddn_last_error()

    def state(self, obj):
        return b"".join(obj.thresholds(c).tobytes() for c in range(B5))

    def oracle(self, runs, outs):
        import orc
        cpu = [orc.OracleP25Rx(lock_symbols=408, use_filter=1) for _ in range(B5)]
        syncs = 0
        for (_, n, xs), o in zip(runs, outs):
            cnt = o[2].view(np.int32)
            rec, fl = o[0].reshape(B5, -1, 10), o[1].reshape(B5, -1)
            for c in range(B5):
                sym, rec4, flo = cpu[c].run(xs[0][c])
                k = int(cnt[c])
                r4, sy = orc.unpack_records10(rec[c, :k])
                assert k == len(sym) and np.array_equal(_f32(sy), _f32(sym)) and np.array_equal(r4, rec4), (self.name, c)
                assert np.array_equal(fl[c, :k], flo), (self.name, c)
                syncs += int(np.count_nonzero(flo & 2)) if o is outs[-1] else 0
        assert syncs > 0                                 # the last call holds a sync


class Fsk4RxStage(Stage):
    """24000 samples of the capture slice tests/test_nonfinite_gpu.py uses, cut at 8000"""
    name, lens = "ddn_fsk4_rx_run", (8000, 16000)

    def __init__(self, proto_name, use_filter):
        self.proto_name, self.use_filter, self.grows = proto_name, use_filter, bool(use_filter)

    def _case(self):
        import rx4
        cap, lpf, self.p, self.proto = (("iq_dmr_t3_ras_cc.npz", 2, rx4.PROTO_DMR, ddn.FSK4_DMR) if self.proto_name == "dmr" else
                                        ("iq_nxdn48.npz", 1, rx4.PROTO_NXDN48, ddn.FSK4_NXDN48))
        return rx4.capture_disc(cap, lpf)

    def make(self):
        self._case()
        rx = ddn.Fsk4Rx(B5, self.proto, use_matched_filter=self.use_filter)
        assert ddn.lib().ddn_fsk4_rx_set_channels_per_wave(rx.h, 8) == 0
        return rx

    def gen(self, seed, k, n):
        """the slice from sample 61000 - 1500 on, shifted by `seed`; call 0 takes its head and call 1 goes on where a first call of the
        shorter length ends, so that the calls of a case are one stream"""
        disc = self._case()
        at = 59500 + 40 * (seed % 50) + (0 if k == 0 else self.lens[0])
        return [np.stack([disc[at + 37 * c:at + 37 * c + n] for c in range(B5)]).astype(np.float32)]

    def plan(self, obj, n):
        l = ddn.lib()
        ms, my = l.ddn_fsk4_rx_max_symbols(obj.h, n), l.ddn_fsk4_rx_max_syncs(obj.h, n)
        return [B5 * ms * 10, B5 * ms, B5 * ms * 2, B5 * 4, B5 * my * 4, B5 * my, B5 * my * ddn.FSK4_PRE, B5 * my * ddn.FSK4_PRE, B5 * 4]

    def launch(self, obj, ins, n, outs, stream):
        l = ddn.lib()
        ms, my = l.ddn_fsk4_rx_max_symbols(obj.h, n), l.ddn_fsk4_rx_max_syncs(obj.h, n)
        rec, fl, pay, cnt, spos, spat, pre, prel, ns = outs
        assert l.ddn_fsk4_rx_run(obj.h, ins[0], n, rec, fl, pay, cnt, ms, spos, spat, pre, prel, ns, my, stream) == 0, l.ddn_last_error()

    def state(self, obj):
        return b"".join(obj.thresholds(c).tobytes() for c in range(B5))

    def oracle(self, runs, outs):
        import rx4
        from test_rx4_gpu import check_channel
        cpu = [rx4.OracleFsk4Rx(rx4.profile(self.p, use_filter=self.use_filter)) for _ in range(B5)]
        n_sync = 0
        for (_, n, xs), o in zip(runs, outs):
            got = dict(rec=o[0].reshape(B5, -1, 10), fl=o[1].reshape(B5, -1), pay=o[2].reshape(B5, -1, 2), cnt=o[3].view(np.int32),
                       sync_pos=o[4].view(np.int32).reshape(B5, -1), sync_pat=o[5].reshape(B5, -1),
                       pre=o[6].reshape(B5, -1, ddn.FSK4_PRE), pre_rel=o[7].reshape(B5, -1, ddn.FSK4_PRE), n_sync=o[8].view(np.int32))
            for c in range(B5):
                want = cpu[c].run(xs[0][c], max_sync=got["sync_pos"].shape[1])
                check_channel(got, c, want)
                n_sync += len(want["sync_pos"]) if o is outs[-1] else 0
        assert n_sync > 0                                # the last call holds a sync


class CqpskStage(Stage):
    name, reset_name, lens, blk, grows = "ddn_cqpsk_run", "ddn_cqpsk_batch_reset", (2503, 3457), 4096, True

    def make(self):
        return ddn.CqpskBatch(B5, block_len=self.blk)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import orc
        return [np.ascontiguousarray(orc.synth_dqpsk_f32(seed, B5, n // 5 + 9, 5)[:, :n])]

    def plan(self, obj, n):
        return [B5 * ddn.lib().ddn_cqpsk_max_symbols(obj.h, n) * 4, B5 * 4]

    def launch(self, obj, ins, n, outs, stream):
        l = ddn.lib()
        assert l.ddn_cqpsk_run(obj.h, ins[0], n, outs[0], l.ddn_cqpsk_max_symbols(obj.h, n), outs[1], stream) == 0, l.ddn_last_error()

    def reset(self, obj, stream):
        assert ddn.lib().ddn_cqpsk_batch_reset(obj.h, stream) == 0

    def state(self, obj):
        return b"".join(obj.state(c).tobytes() for c in range(B5))

    def oracle(self, runs, outs):
        import orc
        cpu = [orc.OracleCqpskFe(rate=24000) for _ in range(B5)]
        for (_, n, xs), o in zip(runs, outs):
            sym, cnt = o[0].view(np.float32).reshape(B5, -1), o[1].view(np.int32)
            for c in range(B5):
                want = cpu[c].run(xs[0][c], self.blk)
                assert cnt[c] == len(want) > 0 and np.array_equal(_f32(sym[c, :cnt[c]]), _f32(want)), (self.name, c)


class GardnerStage(Stage):
    """sps 5: the ring kernel, sps 25: the classic delay-line kernel (tests/test_reset_gpu.py)"""
    name, reset_name, lens = "ddn_gardner_run", "ddn_ted_batch_reset", (1501, 2404)

    def __init__(self, sps):
        self.sps = sps

    def make(self):
        from test_ted_gpu import GpuTed
        return GpuTed(B5, self.sps, 4800)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import orc
        return [np.ascontiguousarray(orc.synth_qpsk_f32(seed, B5, n // self.sps + 20, self.sps, noise=0.08)[:, :n])]

    def plan(self, obj, n):
        return [B5 * (n // 2 + 8) * 8, B5 * 4]

    def launch(self, obj, ins, n, outs, stream):
        l = ddn.lib()
        assert l.ddn_gardner_run(obj.h, ins[0], n, outs[0], n // 2 + 8, outs[1], stream) == 0, l.ddn_last_error()

    def reset(self, obj, stream):
        assert ddn.lib().ddn_ted_batch_reset(obj.h, stream) == 0

    def state(self, obj):
        return b"".join(obj.state(c).tobytes() for c in range(B5))

    def oracle(self, runs, outs):
        import orc
        cpu = [orc.OracleTed(self.sps, 4800) for _ in range(B5)]
        for (_, n, xs), o in zip(runs, outs):
            sym, cnt = o[0].view(np.float32).reshape(B5, -1, 2), o[1].view(np.int32)
            for c in range(B5):
                want = cpu[c].block(xs[0][c])
                assert cnt[c] == len(want) > 0 and np.array_equal(_f32(sym[c, :cnt[c]]), _f32(want)), (self.name, self.sps, c)


class SlicerStage(Stage):
    """call lengths on both sides of 256: the sequential kernel, then the parallel path"""
    name, lens = "ddn_p25_slicer_run", (100, 600)

    def make(self):
        from test_slicer_gpu import GpuSlicer
        return GpuSlicer(B5, 0)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import orc
        return [np.stack([orc.synth_c4fm_symbols(seed * 16 + c, n, scale=0.8 + 0.01 * c, noise=500) for c in range(B5)]).astype(np.float32)]

    def plan(self, obj, n):
        return [B5 * n * 10]

    def launch(self, obj, ins, n, outs, stream):
        assert ddn.lib().ddn_p25_slicer_run(obj.h, ins[0], n, outs[0], stream) == 0, ddn.lib().ddn_last_error()

    def state(self, obj):
        return b"".join(obj.thresholds(c).tobytes() for c in range(B5))

    def oracle(self, runs, outs):
        import orc
        from test_reset_gpu import _slicer_oracle
        want, _ = _slicer_oracle(np.concatenate([xs[0] for _, _, xs in runs], axis=1), 0)
        got = np.concatenate([o[0].reshape(B5, n, 10) for (_, n, _), o in zip(runs, outs)], axis=1)
        assert np.array_equal(orc.unpack_records10(got)[0], want), self.name


class MatchedFilterStage(SlicerStage):
    name, lens = "ddn_p25_matched_filter_run", (100, 600)

    def plan(self, obj, n):
        return [B5 * n * 4]

    def launch(self, obj, ins, n, outs, stream):
        assert ddn.lib().ddn_p25_matched_filter_run(obj.h, ins[0], n, outs[0], stream) == 0, ddn.lib().ddn_last_error()

    def state(self, obj):
        return b""

    def oracle(self, runs, outs):
        import orc
        want = orc.oracle_p25_filter(np.concatenate([xs[0] for _, _, xs in runs], axis=1))
        got = np.concatenate([o[0].view(np.float32).reshape(B5, n) for (_, n, _), o in zip(runs, outs)], axis=1)
        assert np.array_equal(_f32(got), _f32(want)), self.name


class ResamplerStage(Stage):
    name, reset_name, lens = "ddn_resampler_run", "ddn_resampler_reset", (333, 567)

    def make(self):
        from test_resampler_gpu import GpuResampler
        return GpuResampler(B5, 3, 5)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        rng = np.random.default_rng(seed)
        return [(rng.normal(0, 9000, (B5, n)) + 12000 * np.sin(np.arange(n) * 0.07)).astype(np.float32)]

    def plan(self, obj, n):
        return [B5 * (ddn.lib().ddn_resampler_out_len(obj.h, n) + 3) * 4]

    def launch(self, obj, ins, n, outs, stream):
        """(the output length depends on the polyphase index the calls before left: the host knows it without a device wait)"""
        l = ddn.lib()
        k = l.ddn_resampler_out_len(obj.h, n)
        obj.lens = getattr(obj, "lens", []) + [k]
        assert l.ddn_resampler_run(obj.h, ins[0], n, outs[0], k + 3, stream) == 0, l.ddn_last_error()

    def reset(self, obj, stream):
        assert ddn.lib().ddn_resampler_reset(obj.h, stream) == 0

    def state(self, obj):
        return repr((obj.lens, [ddn.lib().ddn_resampler_out_len(obj.h, k) for k in range(12)])).encode()

    def oracle(self, runs, outs):
        import orc
        cpu = [orc.OracleResampler(3, 5) for _ in range(B5)]
        for (_, n, xs), o in zip(runs, outs):
            got = o[0].view(np.float32).reshape(B5, -1)
            for c in range(B5):
                want = cpu[c].run(xs[0][c])
                assert len(want) == got.shape[1] - 3 and np.array_equal(_f32(got[c, :len(want)]), _f32(want)), (self.name, c)


class CqRxStage(Stage):
    """P25 Phase 1 control-channel traffic (tests/test_cqrx_gpu.py) in rows of equal length; the event lists are the object's own
    device buffers, read after the stream has drained"""
    name, reset_name, lens, E = "ddn_cq_rx_run", "ddn_cq_rx_reset", (900, 1700), 256

    def make(self):
        return ddn.CqRx(B5, ddn.CQ_P25P1, 0, 0.0, max_events=self.E)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        from test_cqrx_gpu import p1_traffic, symbols_of
        rng = np.random.default_rng(seed)
        rows = []
        for c in range(B5):
            d = p1_traffic(rng, "ctrl")
            d = np.concatenate([d, rng.integers(0, 4, max(0, n - len(d)))])[:n]
            rows.append(symbols_of(d, rng, noise=0.25, map_idx=(0, 0, 3, 0, 4)[c], invert=c == 1))
        return [np.stack(rows)]

    def plan(self, obj, n):
        return [B5 * n * 10, B5 * n, B5 * 4]

    def launch(self, obj, ins, n, outs, stream):
        l = ddn.lib()
        assert l.ddn_cq_rx_run(obj.h, ins[0], None, n, n, outs[0], outs[1], outs[2], n, stream) == 0, l.ddn_last_error()

    def reset(self, obj, stream):
        assert ddn.lib().ddn_cq_rx_reset(obj.h, stream) == 0

    def state(self, obj):
        """the carried state and the event list of the last call (rows up to its count)"""
        l = ddn.lib()
        ev, nev, evd = np.zeros((B5, self.E, 4), np.int32), np.zeros(B5, np.int32), np.zeros((B5, self.E, 4), np.int32)
        for a, p in ((ev, obj.d_ev), (nev, obj.d_nev), (evd, obj.d_evd)):
            assert l.ddn_device_download(a.ctypes.data, p, a.nbytes) == 0
        rows = b"".join(ev[c, :min(int(nev[c]), self.E)].tobytes() + evd[c, :min(int(nev[c]), self.E)].tobytes() for c in range(B5))
        return b"".join(obj.state(c).tobytes() for c in range(B5)) + nev.tobytes() + rows

    def oracle(self, runs, outs):
        import orc
        cpu = [orc.OracleCqRx(orc.CQ_P25P1, -1, -100.0) for _ in range(B5)]
        syncs = 0
        for (_, n, xs), o in zip(runs, outs):
            rec, fl, cnt = o[0].reshape(B5, n, 10), o[1].reshape(B5, n), o[2].view(np.int32)
            for c in range(B5):
                wr, wf = cpu[c].run(xs[0][c])
                assert cnt[c] == n and np.array_equal(fl[c] & 0x7F, wf) and np.array_equal(rec[c, :, 0].astype(np.int32), wr[:, 0]), (self.name, c)
                assert np.array_equal(rec[c, :, 6:10].copy().view(np.uint32).reshape(-1), _f32(xs[0][c])), (self.name, c)
                syncs += int(((wf & 2) != 0).sum())
        assert syncs > 0


class MbeSynthStage(Stage):
    """`n` counts frames per talk path; the second call is longer, so the record buffer is replaced"""
    name, reset_name, lens, S, grows = "ddn_mbe_synth_batch", "ddn_mbe_batch_reset", (3, 4), B5, True

    def __init__(self, codec_name):
        self.codec_name = codec_name

    def codec(self):
        return ddn.MBE_IMBE if self.codec_name == "imbe" else ddn.MBE_AMBE

    def make(self):
        from test_mbe_gpu import GpuVocoder
        return GpuVocoder(self.codec(), self.S)

    def gen(self, seed, k, n):
        seed = seed + 17 * k
        import mbe
        from test_reset_gpu import _errors, _finish
        rng = np.random.default_rng(seed)
        gen = mbe.random_imbe_bits if self.codec() == ddn.MBE_IMBE else mbe.random_ambe_bits
        return [np.ascontiguousarray(gen(rng, (self.S, n)), np.uint8), _finish(_errors(rng, (self.S, n)))]

    def plan(self, obj, n):
        return [self.S * n * 160 * 4, self.S * n * 5 * 4]

    def launch(self, obj, ins, n, outs, stream):
        assert ddn.lib().ddn_mbe_synth_batch(obj.h, ins[0], ins[1], n, outs[0], outs[1], stream) == 0, ddn.lib().ddn_last_error()

    def reset(self, obj, stream):
        assert ddn.lib().ddn_mbe_batch_reset(obj.h, stream) == 0

    def state(self, obj):
        return b"".join(bytes(p) for s in range(self.S) for p in obj.state(s))

    def oracle(self, runs, outs):
        from test_reset_gpu import _vocoder_oracle
        _, want = _vocoder_oracle(self.codec(), self.S, 0, 0, [(xs[0], xs[1]) for _, _, xs in runs])
        for (_, n, _), o, (pcm, res) in zip(runs, outs, want):
            assert np.array_equal(o[0].view(np.uint32), _f32(pcm).reshape(-1)), (self.name, self.codec_name)
            assert np.array_equal(o[1].view(np.int32), res.reshape(-1)), (self.name, self.codec_name)


class MbeFirstStage(MbeSynthStage):
    """ddn_mbe_batch_set_first_stream numbers the talk paths from 1000 and resets the object on the stream"""
    reset_name, first = "ddn_mbe_batch_set_first_stream", 1000

    def reset(self, obj, stream):
        assert ddn.lib().ddn_mbe_batch_set_first_stream(obj.h, self.first, stream) == 0

    def oracle_after_reset(self, runs, outs):
        from test_reset_gpu import _vocoder_oracle
        calls = [(xs[0], xs[1]) for _, _, xs in runs]
        _, want = _vocoder_oracle(self.codec(), self.S, self.first, 0, calls)
        assert not np.array_equal(want[0][0], _vocoder_oracle(self.codec(), self.S, 0, 0, calls)[1][0][0])     # the numbering shows
        for o, (pcm, res) in zip(outs, want):
            assert np.array_equal(o[0].view(np.uint32), _f32(pcm).reshape(-1)) and np.array_equal(o[1].view(np.int32), res.reshape(-1))


STAGES = {
    "front_end": FrontEnd(), "front_end_halfband": FrontEndHalfband(), "front_end_segments": FrontEndSegments(), "fm_audio": FmAudioStage(), "p25_rx": P25RxStage(),
    "fsk4_rx_dmr_filter": Fsk4RxStage("dmr", 1), "fsk4_rx_nxdn48_plain": Fsk4RxStage("nxdn48", 0), "cqpsk": CqpskStage(),
    "cq_rx": CqRxStage(), "gardner_sps5": GardnerStage(5), "gardner_sps25": GardnerStage(25), "slicer": SlicerStage(),
    "matched_filter": MatchedFilterStage(), "resampler": ResamplerStage(), "mbe_imbe": MbeSynthStage("imbe"), "mbe_ambe": MbeSynthStage("ambe"),
    "mbe_imbe_first": MbeFirstStage("imbe"),
}
DRIVEN.update(s.name for s in STAGES.values())
DRIVEN.update(s.reset_name for s in STAGES.values() if s.reset_name)


def _ops(st, seed, lens, reset_first=False):
    ops = [("reset",)] if reset_first else []
    return ops + [("run", n, st.gen(seed, k, n)) for k, n in enumerate(lens)]


def _solo(st, ops, obj=None, close=True):
    """the reference run -> ([the output buffers of every run as uint8 arrays], the readable state); close=False keeps the object"""
    import torch
    obj = obj or st.make()
    outs = []
    for op in ops:
        if op[0] == "reset":
            st.reset(obj, None)
        else:
            _, n, xs = op
            d = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).cuda() for x in xs]
            o = [torch.full((max(b, 1),), so.MARKER, dtype=torch.uint8, device="cuda") for b in st.plan(obj, n)]
            torch.cuda.synchronize()
            st.launch(obj, [t.data_ptr() for t in d], n, [t.data_ptr() for t in o], None)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy() for t in o])
        torch.cuda.synchronize()
    state = st.state(obj)
    if close:
        st.close(obj)
    return outs, state


class _Queued:
    """the operations of one object behind one late producer: every run's inputs are produced late, from decoys of another seed"""

    def __init__(self, st, obj, ops, decoy_seed):
        self.st, self.obj, self.p, self.steps = st, obj, so.Late(), []
        k = 0
        for op in ops:
            if op[0] == "reset":
                self.steps.append(op)
                continue
            _, n, xs = op
            ins = [self.p.input(x, d) for x, d in zip(xs, st.gen(decoy_seed, k, n))]
            self.steps.append(("run", n, ins, None))
            k += 1
        self.at = 0

    def issue(self, count=None):
        """the next `count` operations (all that are left by default) on the producer's stream.  The output buffers are sized when
        their call is issued, as a host would (an object may size them from what the calls before left): made before begin() where
        the object allows it"""
        for k in range(self.at, len(self.steps) if count is None else self.at + count):
            step = self.steps[k]
            if step[0] == "reset":
                self.st.reset(self.obj, self.p.handle)
            else:
                _, n, ins, outs = step
                self.st.launch(self.obj, [t.data_ptr() for t in ins], n, [t.data_ptr() for t in outs], self.p.handle)
            self.at = k + 1

    def outputs(self, sizes):
        """sizes: per run, the bytes of every output buffer (the solo run's)"""
        runs = [k for k, s in enumerate(self.steps) if s[0] == "run"]
        for k, sz in zip(runs, sizes):
            _, n, ins, _ = self.steps[k]
            self.steps[k] = ("run", n, ins, [self.p.output(b) for b in sz])

    def result(self):
        outs = [[self.p.kept(t) for t in s[3]] for s in self.steps if s[0] == "run"]
        state = self.st.state(self.obj)
        self.st.close(self.obj)
        return outs, state


def _same(st, got, want, tag):
    (go, gs), (wo, ws) = got, want
    assert len(go) == len(wo)
    for k, (g, w) in enumerate(zip(go, wo)):
        for j, (a, b) in enumerate(zip(g, w)):
            assert a.shape == b.shape and np.array_equal(a, b), (st.name, tag, "run %d output %d" % (k, j), np.flatnonzero(a != b)[:8])
    assert gs == ws, (st.name, tag, "state")


def _runs(ops):
    return [op for op in ops if op[0] == "run"]


def _premise(q, name, grows):
    """a call that replaces a buffer of the object waits for its stream on the host first (GROWS_ON_HOST): the premise is then
    asserted in the cases that do not grow anything"""
    assert not q.st.grows or q.st.name in so.GROWS_ON_HOST
    q.p.finish(name, premise=not (grows and q.st.grows))


@gpu
@pytest.mark.parametrize("key", sorted(STAGES))
def test_stage_two_consecutive_calls_the_second_longer(built, key):
    st = STAGES[key]
    ops = _ops(st, 40, st.lens)
    want = _solo(st, ops)
    st.oracle(_runs(ops), want[0])
    assert all((np.concatenate(o) != so.MARKER).any() for o in want[0])
    q = _Queued(st, st.make(), ops, 900)
    q.outputs([[len(a) for a in o] for o in want[0]])
    q.p.begin()
    q.issue()
    _premise(q, st.name, grows=True)
    q.p.wait()
    _same(st, q.result(), want, "consecutive")


@gpu
@pytest.mark.parametrize("key", sorted(k for k, s in STAGES.items() if s.reset_name))
def test_stage_reset_then_run_with_no_host_wait(built, key):
    """the object is dirty from an unrelated input as long as the run (nothing grows afterwards); the delay, the reset and the run are
    queued on `s`; the result is a fresh object's"""
    st = STAGES[key]
    n = st.lens[1]
    ops = _ops(st, 60, (n,))
    want = _solo(st, [("reset",)] + ops)                 # (a reset of a fresh object: what the reset configures is configured)
    st.oracle_after_reset(_runs(ops), want[0])
    dirty_ops = _ops(st, 70, (n,))
    kept = _solo(st, dirty_ops + ops)                    # premise: without the reset the run comes out otherwise
    assert any(not np.array_equal(a, b) for a, b in zip(kept[0][1], want[0][0])) or kept[1] != want[1]
    obj = st.make()
    _solo(st, dirty_ops, obj, close=False)               # (the dirty object lives on)
    st.forget(obj)
    q = _Queued(st, obj, [("reset",)] + ops, 950)
    q.outputs([[len(a) for a in o] for o in want[0]])
    q.p.begin()
    q.issue()
    _premise(q, st.reset_name, grows=False)
    q.p.wait()
    _same(st, q.result(), want, "reset then run")


@gpu
@pytest.mark.parametrize("key", sorted(STAGES))
def test_stage_two_objects_on_two_streams_interleaved(built, key):
    """each object has run one call of the longest length on the null stream before (nothing grows afterwards); then their calls
    alternate on s1 and s2 behind a delay each"""
    import torch
    st = STAGES[key]
    n = st.lens[1]
    qs, wants = [], []
    for k in range(2):
        warm = _ops(st, 80 + k, (n,))
        ops = _ops(st, 90 + 5 * k, (st.lens[0], n))
        want = _solo(st, warm + ops)
        obj = st.make()
        _solo(st, warm, obj, close=False)
        q = _Queued(st, obj, ops, 970 + k)
        q.outputs([[len(a) for a in o] for o in want[0][1:]])
        qs.append(q)
        wants.append(((want[0][1:]), want[1]))
    assert any(not np.array_equal(a, b) for a, b in zip(wants[0][0][0], wants[1][0][0]))
    so.delay_cycles()
    torch.cuda.synchronize()
    for q in qs:
        q.p.begin(settle=False)
    for _ in range(2):
        for q in qs:
            q.issue(1)
    for q in qs:
        _premise(q, st.name, grows=False)
    for q in qs:
        q.p.wait()
    for q, want in zip(qs, wants):
        _same(st, q.result(), want, "two streams")


# ---- the chain objects ---------------------------------------------------------------------------------------------------------------------
# A chain case: make() -> a chain object, calls() -> the I/Q of three consecutive calls (frames lie across their boundaries) or a decoy
# stream of the same kind, snapshot(chain) -> every array of its *_get_results as {name: array}.  The reference is the same object type
# driven on the null stream with a device synchronisation after every call.  The object under test runs its first call the same way (a
# first call sizes the stages' buffers, which waits for the stream: GROWS_ON_HOST) and the others on `s` behind the late producer - d_iq
# is produced late - with no host wait between them; the case synchronises once at the end and takes the snapshot.
I32, U8, U32, F32 = np.int32, np.uint8, np.uint32, np.float32


class ChainCase:
    ops = ("run", "run", "run")     # the first on the null stream; where the object has a flush that takes a stream, that too

    def make(self):
        raise NotImplementedError

    def calls(self, decoy=False):
        raise NotImplementedError

    def op(self, ch, what, d_iq, stream):
        if what == "run":
            ch.run(d_iq, stream)
        else:
            ch.flush(stream)

    def names(self, what):
        return [self.run_name if what == "run" else self.flush_name]


def _fetch_all(ch, r, table):
    return {k: ch.fetch(getattr(r, k), dt, sh) for k, (dt, sh) in table.items() if getattr(r, k)}


class P25Chain(ChainCase):
    """three channels in calls of 6000 samples (tests/test_chain_gpu.py: shorter than a voice frame, every LDU lies across a boundary)"""
    run_name, B, n = "ddn_p25_chain_run", 3, 6000

    def make(self):
        return ddn.P25ChainC(self.B, self.n, max_ldu=4)

    def calls(self, decoy=False):
        from test_chain_gpu import _stream
        iq = _stream(self.B, 3 * self.n)
        iq = np.roll(iq, 1, axis=0) if decoy else iq
        return [np.ascontiguousarray(iq[:, k * self.n:(k + 1) * self.n]) for k in range(3)]

    def snapshot(self, ch):
        import chain_stream
        col = chain_stream.Collector(ch, everything=True)
        col.take()
        out = {}
        for c in range(self.B):
            out["rec%d" % c], out["fl%d" % c] = col.rec[c][0], col.fl[c][0]
            out["events%d" % c], out["event_data%d" % c] = col.events[c][0], col.event_data[c][0]
            for g, d in sorted(col.frames[c].items()):
                for k, v in d.items():
                    if k == "tsbk":
                        v = np.concatenate([np.r_[t, crc] for t, crc in v])
                    out["frame%d@%d.%s" % (c, g, k)] = np.asarray(v)
            for i, v in enumerate(col.voice[c]):
                for j, a in enumerate(v):
                    out["voice%d.%d.%d" % (c, i, j)] = np.asarray(a)
        out["straddles"] = np.array([sum(g < 0 for g in col.frames[c]) for c in range(self.B)])
        return out

    def holds(self, snap):
        return snap["straddles"].sum() > 0               # a frame whose sync lies in the carried tail of the call before


class P25ChainStaged(P25Chain):
    """the three stages of a call as separate calls on the stream"""
    run_name = "ddn_p25_chain_stage"

    def op(self, ch, what, d_iq, stream):
        l = ddn.lib()
        for stage in range(3):
            assert l.ddn_p25_chain_stage(ch.h, stage, d_iq, stream) == 0, l.ddn_last_error()


class DmrMsChain(ChainCase):
    """the DMR section with the MS stage on (tests/test_dmr_ms_chain_gpu.py: two channels of the generated batch in calls of 24000)"""
    run_name, flush_name, B, n = "ddn_fsk4_chain_run", "ddn_fsk4_chain_flush", 2, 24000
    ops = ("run", "run", "run", "flush")

    def make(self):
        ch = ddn.Fsk4ChainC(self.B, self.n, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=1)
        ch.set_dmr_ms(1)
        return ch

    def calls(self, decoy=False):
        import dmrmsgen
        x = dmrmsgen.air_batch()
        assert x.shape[1] >= 3 * self.n
        x = x[4:6] if decoy else x[:2]                   # (every channel has its own delay and noise)
        return [np.ascontiguousarray(x[:, k * self.n:(k + 1) * self.n]) for k in range(3)]

    def snapshot(self, ch):
        from test_dmr_ms_chain_gpu import _main_arrays
        B, r, m = self.B, ch.results(), ch.dmr_ms_results()
        out = _fetch_all(ch, r, _main_arrays(r, B, 1))
        b, d, v = m.bursts, m.data, m.voice
        md, mv, ml = b.max_data, b.max_voice, b.max_lc
        for s, table in ((b, dict(d_n_data=(I32, (B,)), d_n_voice=(I32, (B,)), d_n_lc=(I32, (B,)), d_cc=(I32, (B,)), d_dropped=(I32, (B,)),
                                  d_phase=(I32, (B,)), d_data_start=(I32, (B, md)), d_data_sync=(I32, (B, md)), d_data_pat=(U8, (B, md)),
                                  d_data_slot=(U8, (B, md)), d_data_status=(U8, (B, md)), d_data_cc=(U8, (B, md)), d_voice_start=(I32, (B, mv)),
                                  d_voice_pre=(I32, (B, mv)), d_voice_vc=(U8, (B, mv)), d_voice_tact_ok=(U8, (B, mv)), d_voice_emb_ok=(U8, (B, mv)),
                                  d_voice_emb_cc=(U8, (B, mv)), d_voice_power=(U8, (B, mv)), d_voice_sync48=(U8, (B, mv, 48)),
                                  d_lc_pos=(I32, (B, ml)), d_lc_in128=(U8, (B, ml, 128)))),
                         (d, dict(d_type=(U8, (B, md)), d_info196=(U8, (B, md, 196)), d_bits96=(U8, (B, md, 96)), d_bytes12=(U8, (B, md, 12)),
                                  d_errs=(U32, (B, md)), d_crc=(U8, (B, md)), d_r34_unconfirmed=(U8, (B, md, 18)),
                                  d_r34_confirmed=(U8, (B, md, 18)), d_r34_confirmed_crc=(U8, (B, md)), d_r34_pool_n=(I32, (B, md)))),
                         (v, dict(d_ambe_frames=(U8, (B, mv, 3, 4, 24)), d_skip=(U8, (B, mv, 3)), d_lc77=(U8, (B, ml, 77)), d_lc_errs=(U32, (B, ml)),
                                  d_lc_ok=(U8, (B, ml)), d_ambe_bits=(U8, (B, mv, 3, 49)), d_ambe_result=(I32, (B, mv, 3, 5)),
                                  d_pcm=(F32, (B, mv, 3, 160))))):
            out.update({"ms." + k: a for k, a in _fetch_all(ch, s, table).items()})
        return out

    def holds(self, snap):
        return int(snap["ms.d_n_data"].sum() + snap["ms.d_n_voice"].sum()) > 0 and int(snap["d_n_sync"].sum()) > 0


class NxdnCtrlChain(ChainCase):
    """the NXDN section with the control stage on (tests/test_nxdn_ctrl_chain_gpu.py: NXDN96, calls of 24000)"""
    run_name, flush_name, n = "ddn_fsk4_chain_stage", "ddn_fsk4_chain_flush", 24000
    ops = ("run", "run", "run", "flush")

    def make(self):
        import chain_fsk4_stream as cs
        row = cs.NXDN["nxdn96"]
        ch = ddn.Fsk4ChainC(3, self.n, row["gpu"], rf_mod=row["rf_mod"], handlers=1, vocoder=0)
        ch.set_nxdn_ctrl(1)
        return ch

    def calls(self, decoy=False):
        import nxdngen
        x = nxdngen.air_batch("nxdn96")
        assert x.shape[1] >= 3 * self.n
        x = np.roll(x, 1, axis=0) if decoy else x
        return [np.ascontiguousarray(x[:, k * self.n:(k + 1) * self.n]) for k in range(3)]

    def op(self, ch, what, d_iq, stream):
        """(the three stages as separate calls: ddn_fsk4_chain_run is the DMR case's)"""
        l = ddn.lib()
        if what == "flush":
            return ch.flush(stream)
        for stage in range(3):
            assert l.ddn_fsk4_chain_stage(ch.h, stage, d_iq, stream) == 0, l.ddn_last_error()

    def snapshot(self, ch):
        import nxdn_ctrl as nc
        from test_nxdn_ctrl_chain_gpu import MAIN
        B, r, cr = 3, ch.results(), ch.nxdn_ctrl_results()
        S = int(r.max_syncs)
        out = _fetch_all(ch, r, {k: (dt, (B,) if sh is None else (B, S) + sh) for k, (dt, sh) in MAIN.items()})
        out.update(_fetch_all(ch, r, dict(d_records10=(U8, (B, int(r.stride_symbols), 10)), d_flags=(U8, (B, int(r.stride_symbols))))))
        out.update({"frames." + k: ch.fetch(getattr(cr.frames, "d_" + k), dt, (B, S) + sh) for k, (dt, sh) in nc.FRAME_ARRAYS.items()})
        out.update({"messages." + k: ch.fetch(getattr(cr.messages, "d_" + k), dt, (B, S) + sh) for k, (dt, sh) in nc.MESSAGE_ARRAYS.items()})
        return out

    def holds(self, snap):
        return int(snap["d_n_sync"].sum()) > 0


class P25P2Chain(ChainCase):
    """the reference's Phase 2 capture on three channels in calls of 32000 samples (tests/test_chain_p25p2_gpu.py)"""
    run_name, flush_name, n = "ddn_p25p2_chain_run", "ddn_p25p2_chain_flush", 32000
    ops = ("run", "run", "run", "flush")

    def make(self):
        from test_chain_p25p2_gpu import SEED
        return ddn.P25P2ChainC([SEED, SEED, 0], self.n, vocoder=1)

    def calls(self, decoy=False):
        from conftest import golden
        iq = golden("iq_p25p2_cc.npz")["iq"]
        assert len(iq) >= 3 * self.n
        iq = np.roll(iq, self.n // 2, axis=0)[:3 * self.n] if decoy else iq[:3 * self.n]     # (the decoy: the capture half a call later)
        return [np.ascontiguousarray(np.broadcast_to(iq[k * self.n:(k + 1) * self.n], (3, self.n, 2))) for k in range(3)]

    def snapshot(self, ch):
        r, B = ch.results(), 3
        G, st, cap = int(r.max_groups), int(r.stride_symbols), int(r.voice_frames)
        return _fetch_all(ch, r, dict(d_voice_src=(I32, (2 * B, cap)), d_voice_count=(I32, (2 * B,)), d_voice_bits=(U8, (2 * B, cap, 49)),
                                      d_voice_result=(I32, (2 * B, cap, 5)), d_pcm=(F32, (2 * B, cap, 160)),
                                      d_records10=(U8, (B, st, 10)), d_flags=(U8, (B, st)), d_new=(I32, (B,)), d_counts=(I32, (B,)),
                                      d_n_groups=(I32, (B,)), d_group_pos=(I32, (B, G)), d_dropped_syncs=(I32, (B,)), d_info=(I32, (B, G, 4, 8)),
                                      d_payload=(U8, (B, G, 4, 180)), d_ambe_fr=(U8, (B, G, 4, 384)), d_ambe_rel=(U8, (B, G, 4, 384)),
                                      d_ess=(U8, (B, G, 4, 96))))

    def holds(self, snap):
        return int(snap["d_n_groups"].sum()) > 0


CHAINS = {"p25": P25Chain(), "p25_staged": P25ChainStaged(), "fsk4_dmr_ms": DmrMsChain(), "fsk4_nxdn_ctrl": NxdnCtrlChain(), "p25p2": P25P2Chain()}
for _c in CHAINS.values():
    DRIVEN.update(n for what in _c.ops for n in _c.names(what))
_chain_cases = [(k, ops) for k, c in sorted(CHAINS.items()) for ops in sorted({c.ops[:3], c.ops})]


def _chain_reference(case, ops):
    import torch
    ch = case.make()
    d = [torch.from_numpy(x).cuda() for x in case.calls()]
    torch.cuda.synchronize()
    for k, what in enumerate(ops):
        case.op(ch, what, d[k].data_ptr() if what == "run" else None, None)
        torch.cuda.synchronize()
    snap = case.snapshot(ch)
    ch.close()
    return snap


@gpu
@pytest.mark.parametrize("key,ops", _chain_cases, ids=["%s-%s" % (k, "+".join(o)) for k, o in _chain_cases])
def test_chain_object_behind_a_late_producer(built, key, ops):
    import torch
    case = CHAINS[key]
    want = _chain_reference(case, ops)
    assert case.holds(want) or ops[-1] == "flush"        # (a flush brings no new group: the run-only case holds the traffic)
    warm = case.make()                                   # first-use costs of the kernels (not of the object under test)
    d = [torch.from_numpy(x).cuda() for x in case.calls(decoy=True)]
    torch.cuda.synchronize()
    for k, what in enumerate(ops):
        case.op(warm, what, d[k].data_ptr() if what == "run" else None, None)
    torch.cuda.synchronize()
    warm.close()
    ch = case.make()
    p = so.Late()
    first = torch.from_numpy(case.calls()[0]).cuda()
    live = [None] + [p.input(x, y) for x, y in zip(case.calls()[1:], case.calls(decoy=True)[1:])]
    torch.cuda.synchronize()
    case.op(ch, ops[0], first.data_ptr(), None)
    p.begin()
    blocks = False
    for k, what in list(enumerate(ops))[1:]:
        case.op(ch, what, live[k].data_ptr() if what == "run" else None, p.handle)
        blocks = blocks or any(n in so.BLOCKS_HOST for n in case.names(what))
        if k == 1 and so.BLOCKS_HOST.get(case.run_name) is so.SCRATCH:
            assert p.pending(), case.run_name            # the first call queued on the busy stream returns at once (the second waits)
    p.finish(case.run_name, premise=not blocks)
    p.wait()
    got = case.snapshot(ch)
    ch.close()
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (key, ops, k)


# ---- the chain plumbing of the bindings: every stage a call of the C ABI on the caller's stream --------------------------------------------
# ddn_chain.P25Chain and ddn_chain_fsk4.Fsk4Chain issue the framer, gather, FEC and vocoder calls one by one on the stream they are
# given (and a few torch operations on torch's current stream).  A case runs the first call on the null stream (it sizes the stages'
# buffers), then two calls on `s` behind the late producer with torch's current stream set to `s`; every tensor the object owns must
# equal the same object's driven on the null stream with a device synchronisation after every call.  Several stages of a call take
# stream-ordered scratch, so the premise cannot hold for the call as a whole (stream_order.SCRATCH) and is not asserted here.
PLUMBED = {
    "p25": ("ddn_p25p1_framer_index", "ddn_p25p1_framer_gather_nid", "ddn_p25p1_framer_gather_trellis_block", "ddn_p25p1_framer_gather_r34_block",
            "ddn_p25p1_framer_gather_ldu_words", "ddn_p25p1_framer_pack_ldu_rs", "ddn_p25p1_framer_voice_index", "ddn_p25p1_framer_imbe_index",
            "ddn_mbe_frame_decode_batch", "ddn_mbe_result_skip_batch"),
    "dmr": ("ddn_dmr_burst_gather",),
    "nxdn48": ("ddn_nxdn_frame_gather", "ddn_nxdn_crc_check_batch", "ddn_nxdn_voice_gather"),
}
for _names in PLUMBED.values():
    DRIVEN.update(_names)


def _plumbing(key, torch):
    """-> (the object, the I/Q of three calls, the same of a decoy, holds(object) -> the traffic reached the stages)"""
    import chain_fsk4_stream as cs
    import ddn_chain
    import ddn_chain_fsk4
    if key == "p25":
        from test_chain_gpu import _stream
        B, n = 3, 24000

        class WithTheRest(ddn_chain.P25Chain):
            """(+ the two framer calls the plumbing leaves out: the rate 3/4 block gather and the plain IMBE index)"""

            def frame_fec(self, st):
                ddn_chain.P25Chain.frame_fec(self, st)
                l, t = self.l, (lambda a: a.data_ptr())
                if not hasattr(self, "r34_dib"):
                    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
                    self.r34_dib, self.r34_rel = z((self.S, 98), torch.uint8), z((self.S, 98), torch.uint8)
                    self.first9, self.sc9 = z((self.S * 9,), torch.int64), z((self.S * 9,), torch.int32)
                assert l.ddn_p25p1_framer_gather_r34_block(self.fr, 0, t(self.rec), t(self.cnt), self.ms, t(self.r34_dib), t(self.r34_rel), None, st) == 0
                assert l.ddn_p25p1_framer_imbe_index(self.fr, self.ms, t(self.first9), t(self.sc9), st) == 0

        obj = WithTheRest(torch, B, n, None)
        torch.zeros(1, device="cuda")
        obj.frame_fec(None)                              # (makes the extra tensors before anything is queued)
        torch.cuda.synchronize()
        iq = _stream(B, 3 * n)
        holds = lambda o: int(o.n_ldu.sum()) > 0 and bool(o.pcm.abs().sum() > 0) and int(o.v_nid.sum()) > 0
    else:
        B, n = 3, 20000
        proto = ddn.FSK4_DMR if key == "dmr" else ddn.FSK4_NXDN48
        obj = ddn_chain_fsk4.Fsk4Chain(torch, B, n, proto, rf_mod=2 if key == "dmr" else 0)
        iq = cs.stream(key, "plain" if key == "dmr" else "voice")[:, :3 * n]
        holds = (lambda o: int(o.valid.sum()) > 0) if key == "dmr" else (lambda o: int(o.v_ns.sum()) > 0 and bool(o.pcm.abs().sum() > 0))
    assert iq.shape[1] == 3 * n
    cut = lambda x: [np.ascontiguousarray(x[:, k * n:(k + 1) * n]) for k in range(3)]
    return obj, cut(iq), cut(np.roll(iq, 1, axis=0)), holds


def _tensors(obj, torch):
    out = {}
    for name, v in sorted(vars(obj).items()):
        for j, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            for i, u in enumerate(t if isinstance(t, (list, tuple)) else [t]):
                if torch.is_tensor(u) and u.is_cuda:
                    out["%s.%d.%d" % (name, j, i)] = u.cpu().numpy().tobytes()
    return out


@gpu
@pytest.mark.parametrize("key", sorted(PLUMBED))
def test_binding_chain_plumbing_behind_a_late_producer(built, key):
    import torch
    ref, calls, _, holds = _plumbing(key, torch)
    for x in calls:
        d = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        ref.run(d, None)
        torch.cuda.synchronize()
    assert holds(ref)
    want = _tensors(ref, torch)
    obj, calls, decoys, _ = _plumbing(key, torch)
    first = torch.from_numpy(calls[0]).cuda()
    p = so.Late()
    live = [p.input(x, y) for x, y in zip(calls[1:], decoys[1:])]
    torch.cuda.synchronize()
    obj.run(first, None)
    p.begin()
    with torch.cuda.stream(p.s):
        for t in live:
            obj.run(t, p.handle)
    p.finish("binding chain " + key, premise=False)
    p.wait()
    got = _tensors(obj, torch)
    assert sorted(got) == sorted(want) and len(want) > 10
    for k in sorted(want):
        assert got[k] == want[k], (key, k)


# ---- every section of the fsk4 chain object, with the reference its own chain test uses ----------------------------------------------------
# The chain tests drive their object through chain_fsk4_stream.drive (a call, then the results are read) and compare with the CPU
# oracle of the whole stream.  Here the same tests run with a drive that puts every call, the flush included, behind a late producer
# of its own: the call's I/Q arrives late on `s` over a decoy (the batch with its channels rotated), the call is issued on `s`, and the
# results are read once `s` has drained - the host wait the scheme has after every call.  The premise is not asserted: the decode
# stages take stream-ordered scratch more than once per call (stream_order.SCRATCH).
LATE_DRIVE_MS = 5       # (no premise to hold: the delay only has to outlast the call's own return, 0.3 ms)
_late_calls = []


def _late_drive(ch, x, n, take, info=None):
    B = x.shape[0]
    decoy, news = np.roll(x, 1, axis=0), []
    for k in list(range(x.shape[1] // n)) + ["flush"]:
        p = so.Late()
        if k == "flush":
            p.begin(ms=LATE_DRIVE_MS)
            ch.flush(p.handle)
        else:
            live = p.input(np.ascontiguousarray(x[:, k * n:(k + 1) * n]), np.ascontiguousarray(decoy[:, k * n:(k + 1) * n]))
            p.begin(ms=LATE_DRIVE_MS)
            ch.run(live.data_ptr(), p.handle)
        p.finish("ddn_fsk4_chain_run", premise=False)
        p.wait()
        take()
        news.append(ch.fetch(ch.results().d_new, np.int32, (B,)))
        _late_calls.append(k)
    if info is not None:
        r = ch.results()
        info.update(dropped=ch.fetch(r.d_dropped_syncs, np.int32, (B,)), new=np.stack(news), T=int(r.carry_symbols), max_syncs=int(r.max_syncs))


def _section(name):
    import chain_fsk4_stream as cs
    if name in ("dstar", "edacs", "m17"):
        return lambda: cs.run_and_check(name, "plain", cs.call_size(name, "block"))
    if name == "m17_data":
        import test_m17_data_chain_gpu as t
        return lambda: t.test_streams_through_the_chain_object(True, t.L // 3)
    if name == "dmr_pdu":
        import test_dmr_pdu_chain_gpu as t
        return lambda: t.test_pdu_stream_through_the_chain_object(True, "three")
    import test_chain_fsk4_short_calls_gpu as t                       # the voice sections, vocoder = 1
    return lambda: t.test_short_calls_voice_to_pcm(True, name[:-6])


SECTIONS = ("dstar", "edacs", "m17", "m17_data", "dmr_pdu", "ysf_voice", "dpmr_voice", "dmr_voice", "nxdn48_voice")


@gpu
@pytest.mark.parametrize("name", SECTIONS)
def test_fsk4_chain_section_with_every_call_behind_a_late_producer(built, monkeypatch, name):
    import chain_fsk4_stream as cs
    run = _section(name)
    monkeypatch.setattr(cs, "drive", _late_drive)
    del _late_calls[:]
    run()
    assert len(_late_calls) >= 3 and _late_calls[-1] == "flush"


# ---- the stateless calls without a `_host` twin ------------------------------------------------------------------------------------------------
# The driver of the `_batch` twins over a second table.  The reference is the call itself on the null stream with a device
# synchronisation behind it (the calls' own tests hold that against the restatement at these shapes: tests/test_voice_gather_gpu.py,
# test_p25p2_xcch_gpu.py, test_lsd.py, test_dmr_ms_gpu.py, test_nxdn_ctrl_gpu.py); the deinterleave is held against the restatement here.
def _direct_calls():
    from test_host_staging_gpu import A, I16, I32, U8
    l = ddn.lib()
    n, B, ms, mb = 7, 5, 900, 7
    return {
        "ddn_ambe2450_deinterleave_batch": [A("in", U8, n * 36, 0, 4), A("in", U8, n * 36, 0, 256), n, A("out", U8, n * 96), A("out", U8, n * 96)],
        "ddn_dmr_voice_burst_gather": [A("in", U8, B * ms * 10, 0, 256), A("in", I32, B, np.array([900, 650, 143, 400, 0])), ms,
                                       A("in", I32, B * mb, -20, 800), B, mb, 0, A("out", U8, B * mb * 288), A("out", U8, B * mb * 288),
                                       A("out", U8, B * mb * 48), A("out", U8, B * mb * 24), A("out", U8, B * mb)],
        "ddn_p25p2_voice_frames_batch": [A("in", U8, n * 360, 0, 2), A("in", I16, n * 360, -400, 400), n, 4, A("out", U8, n * 384), A("out", U8, n * 384)],
        "ddn_fec_p25_tsbk_select_batch": [A("in", U8, 5 * 8 * 16, 0, 256), A("in", I32, 5, 0, 9), 5, A("out", U8, 60), A("out", U8, 5), A("out", U8, 5)],
        "ddn_dmr_ms_state_init": [A("out", U8, 3 * l.ddn_dmr_ms_state_bytes()), 3],
        "ddn_nxdn_ctrl_state_init": [A("out", U8, 3 * l.ddn_nxdn_ctrl_state_bytes()), 3],
    }


DIRECT = ("ddn_ambe2450_deinterleave_batch", "ddn_dmr_voice_burst_gather", "ddn_p25p2_voice_frames_batch", "ddn_fec_p25_tsbk_select_batch",
          "ddn_dmr_ms_state_init", "ddn_nxdn_ctrl_state_init")
DRIVEN.update(DIRECT)


class _Direct:
    def __init__(self, name, seed):
        import torch
        self.name, spec = name, _direct_calls()[name]
        self.vals, decoy = _draw_spec(spec, seed), _draw_spec(spec, seed + 500)
        self.want = self._null_stream(self.vals)
        self.decoy_want = self._null_stream(decoy)
        self.p, self.buf = so.Late(), {}
        for k, ((a, v), (_, d)) in enumerate(zip(self.vals, decoy)):
            if v is not None:
                self.buf[k] = self.p.output(v.nbytes) if a[0] == "out" else self.p.input(v, d)
        torch.cuda.synchronize()

    def _null_stream(self, vals):
        import torch
        buf = {k: torch.from_numpy(v.view(np.uint8).copy()).cuda() for k, (a, v) in enumerate(vals) if v is not None}
        for k, (a, v) in enumerate(vals):
            if v is not None and a[0] == "out":
                buf[k].fill_(so.MARKER)
        torch.cuda.synchronize()
        assert getattr(ddn.lib(), self.name)(*_batch_args(vals, buf, None)) == 0, ddn.lib().ddn_last_error()
        torch.cuda.synchronize()
        return {k: buf[k].cpu().numpy() for k, (a, v) in enumerate(vals) if v is not None and a[0] == "out"}

    def issue(self):
        assert getattr(ddn.lib(), self.name)(*_batch_args(self.vals, self.buf, self.p.handle)) == 0, ddn.lib().ddn_last_error()

    def check(self):
        for k, w in self.want.items():
            assert (w != so.MARKER).any() and np.array_equal(self.p.kept(self.buf[k]), w), (self.name, k)


def _draw_spec(spec, seed):
    rng = np.random.default_rng(seed)
    vals = []
    for a in spec:
        if not _is_ptr(a):
            vals.append((a, None))
            continue
        role, dtype, count, lo, hi = a
        v = lo.astype(dtype) if isinstance(lo, np.ndarray) else rng.integers(lo, hi, count).astype(dtype)
        vals.append((a, np.zeros(count, dtype) if role == "out" else v))
    return vals


@gpu
@pytest.mark.parametrize("name", DIRECT)
def test_stateless_call_without_a_host_twin_behind_a_late_producer(built, name):
    import torch
    c = _Direct(name, 400 + DIRECT.index(name))
    if not name.endswith("_state_init"):
        assert any(not np.array_equal(c.want[k], c.decoy_want[k]) for k in c.want), "the decoy's result equals the true one"
    if name == "ddn_ambe2450_deinterleave_batch":
        import rx4
        dib, rel = c.vals[0][1].reshape(-1, 36), c.vals[1][1].reshape(-1, 36)
        for i in range(len(dib)):
            w = rx4.ambe2450_deinterleave(dib[i], rel[i])
            assert np.array_equal(c.want[3].reshape(-1, 4, 24)[i], w[0]) and np.array_equal(c.want[4].reshape(-1, 4, 24)[i], w[1])
    c.p.begin()
    c.issue()
    c.p.finish(name)
    c.p.wait()
    c.check()
    a, b = _Direct(name, 600 + DIRECT.index(name)), _Direct(name, 700 + DIRECT.index(name))      # two streams at once
    so.delay_cycles()
    torch.cuda.synchronize()
    for q in (a, b):
        q.p.begin(settle=False)
    for q in (a, b):
        q.issue()
    for q in (a, b):
        q.p.finish(name)
    for q in (a, b):
        q.p.wait()
        q.check()


@gpu
def test_the_measured_host_times_stay_inside_the_delay(built):
    """what the cases above measured between the end of the producer's copies and the return of their last call, where the premise
    was asserted (run last in the module; prints the table the delay is sized from)"""
    rows = sorted(so.HOST_MS.items(), key=lambda kv: -kv[1])
    for name, ms in rows[:12]:
        print("%8.2f ms  %s" % (ms, name))
    assert not rows or 4 * rows[0][1] < so.DELAY_MS


# ---- completeness (CPU) --------------------------------------------------------------------------------------------------------------------
# {callee: the driven call above that passes its own stream on to it}; the callee's name occurs in the file that defines the caller
_P25 = "ddn_p25_chain_run"            # the decode stage of the P25 Phase 1 chain: HDU / TDULC words, low speed data
_FSK4 = "ddn_fsk4_chain_run"          # the sections of the fsk4 chain: the DMR section with the MS stage on, and SECTIONS above
_NXDN = "ddn_fsk4_chain_stage"        # the NXDN section with the control stage on
REACHED_ON_STREAM = {
    "ddn_p25p1_framer_gather_hdu": _P25, "ddn_p25p1_framer_pack_hdu_rs": _P25, "ddn_p25p1_framer_gather_tdulc": _P25,
    "ddn_p25p1_framer_pack_tdulc_rs": _P25, "ddn_p25p1_framer_gather_lsd": _P25,
    "ddn_dmr_ms_walk_batch": _FSK4, "ddn_dmr_ms_data_batch": _FSK4, "ddn_dmr_ms_voice_batch": _FSK4,
    "ddn_dmr_pdu_marks_batch": _FSK4, "ddn_dmr_pdu_walk_batch": _FSK4,
    "ddn_m17_lsf_decode_batch": _FSK4, "ddn_m17_str_decode_batch": _FSK4, "ddn_m17_lich_assemble_batch": _FSK4,
    "ddn_m17_pkt_decode_batch": _FSK4, "ddn_m17_brt_decode_batch": _FSK4, "ddn_m17_data_assemble_batch": _FSK4,
    "ddn_ysf_fich_decode_batch": _FSK4, "ddn_ysf_payload_decode_batch": _FSK4,
    "ddn_dpmr_superframe_decode_batch": _FSK4, "ddn_dpmr_identity_batch": _FSK4, "ddn_dpmr_voice_gather": _FSK4,
    "ddn_dstar_header_decode_batch": _FSK4, "ddn_dstar_voice_decode_batch": _FSK4, "ddn_edacs_frame_decode_batch": _FSK4,
    "ddn_nxdn_ctrl_decode_batch": _NXDN, "ddn_nxdn_ctrl_walk_batch": _NXDN,
    "ddn_p25p2_scramble_bits_batch": "ddn_p25p2_groups_batch", "ddn_p25p2_descramble_batch": "ddn_p25p2_groups_batch",
}


def test_every_stream_taking_export_is_covered():
    from test_cabi_called import _words, defining_source
    takers = so.stream_takers(os.path.join(ddn.ROOT, "include"))
    assert len(takers) > 100 and "ddn_fsk4_rx_run" in takers and "ddn_fec_bptc_16x2_batch" in takers
    assert all(n in ddn.PROTOTYPES for n in takers)
    known = DRIVEN | set(REACHED_ON_STREAM)
    missing = sorted(n for n in takers if n not in known)
    assert not missing, missing
    stale = sorted(n for n in known if n not in takers)
    assert not stale, stale
    twice = sorted(n for n in DRIVEN if n in REACHED_ON_STREAM)
    assert not twice, twice
    with open(os.path.abspath(__file__)) as f:
        me = _words(f.read())
    for n in sorted(DRIVEN):
        assert n in me or n[:-6] + "_host" in CALLS, n
    for callee, caller in sorted(REACHED_ON_STREAM.items()):
        assert caller in DRIVEN, (callee, caller)
        src = defining_source(caller)
        assert src is not None, caller
        body = re.sub(r"^%s\(" % re.escape(callee), "", src, flags=re.M)
        assert callee in _words(body), (callee, caller)


def test_blocking_calls_are_named_with_the_line_that_waits():
    csrc = os.path.join(ddn.ROOT, "dsd-neo_amd", "csrc")
    takers = so.stream_takers(os.path.join(ddn.ROOT, "include"))
    for name, (fn, lines) in list(so.BLOCKS_HOST.items()) + list(so.GROWS_ON_HOST.items()):
        assert name in takers and name in DRIVEN, name
        with open(os.path.join(csrc, fn)) as f:
            assert " ".join(lines.split()) in " ".join(f.read().split()), (name, fn, lines)
