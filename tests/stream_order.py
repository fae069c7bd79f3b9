"""The late producer: the harness of tests/test_stream_order_gpu.py.  TEST INFRASTRUCTURE - never imported by the product.

A call that is "asynchronous on `hip_stream`" may rely on nothing but stream order.  The harness makes stream order the only thing
that holds: on one non-blocking stream `s` (it does not synchronise with the null stream) it queues

  1. a delay kernel (torch.cuda._sleep) and an event behind it,
  2. device-to-device copies of the true inputs into the live input buffers, which until then hold a decoy (valid input of the
     same kind and range from another seed: counts and indices stay valid, nothing can fault),
  3. the call under test,
  4. copies of its outputs (marker bytes until then) into keep buffers,
  5. the decoy back over the inputs and the marker back over the outputs,

and returns to the host while the event of step 1 is still pending (`not ev.query()`: the premise, asserted, never skipped).  A
kernel, memset or copy of the call that runs on another stream, or a host copy in the middle of it, sees the decoy or writes where
step 5 overwrites it, and the keep buffers differ from the reference.

The delay is a condition, not a tolerance.  Measured on an MI355X after a warm-up call on the null stream, the longest host-side
time from the end of step 2 to the return of the last call of a case, over every case whose calls do not wait on the host
(BLOCKS_HOST / GROWS_ON_HOST list those that do), was %(MEASURED_MS).2f ms (%(MEASURED_AT)s).  Times a margin of 4 for host jitter on a
shared machine that is %(MARGIN_MS).1f ms; the delay is %(DELAY_MS)d ms, which also covers what the harness itself queues between the
delay kernel and the call (a dozen copies through torch).  The premise assertion keeps the figure honest: a call that outlasts the
delay fails its test."""
import ctypes as C
import re
import time

import numpy as np

MEASURED_MS = 0.34
MEASURED_AT = "two calls of ddn_p25_chain_run; 0.29 and 0.34 ms in two runs; a single stage call stays below 0.3 ms"
DELAY_MS = 40
MARKER = 0xA5
HIP_STREAM_NON_BLOCKING = 1

__doc__ = __doc__ % dict(MEASURED_MS=MEASURED_MS, MEASURED_AT=MEASURED_AT, MARGIN_MS=4 * MEASURED_MS, DELAY_MS=DELAY_MS)
assert DELAY_MS >= 4 * MEASURED_MS

# calls that wait for their stream on the host by design: the premise cannot hold, their results are checked all the same.
# {name: (source file, the lines that wait, white space collapsed)}
SCRATCH = ("ddn_api_util.h", "for (int i = 0; i < n; i++) { (void)hipFreeAsync(p[i], st); }")
_GROUPS = ("ddn_api_p25p2.cpp", "HIP_TRY(hipStreamSynchronize(st)); const int n_f = h_counts[0],")   # it reads its four list lengths
BLOCKS_HOST = {
    "ddn_p25p2_groups_batch": _GROUPS,
    "ddn_p25p2_chain_run": ("ddn_api_p25p2_chain.cpp", "DDN_TRY(ddn_p25p2_groups_batch(c->d_bits, c->d_llr,"),     # (through the call above)
    "ddn_p25p2_chain_flush": ("ddn_api_p25p2_chain.cpp", "DDN_TRY(p2_decode(c, cur, 1, st)); HIP_TRY(hipStreamSynchronize(st));"),
    "ddn_fsk4_chain_flush": ("ddn_api_chain_fsk4.cpp", "c->step++; HIP_TRY(hipStreamSynchronize(st)); return DDN_OK;"),
    # the MS and the control stage take stream-ordered scratch (DdnScratch) in every call.  Measured on the MI355X (ROCm 7.0): the
    # second hipFreeAsync queued on a stream whose earlier work has not finished waits for that work in the runtime (39.8 ms behind
    # a delay of 40 ms; the first returns in 0.01 ms).  So the first call queued behind the producer returns at once and the second
    # waits: any two scratch-taking calls in a row on one busy stream do.
    "ddn_fsk4_chain_run": SCRATCH,
    "ddn_fsk4_chain_stage": SCRATCH,
}

# calls that wait for their stream on the host only when a longer call than any before makes them replace a buffer of the object
# (first use included): {name: (source file, the line that waits)}.  Their premise is asserted in the cases where nothing grows.
_LPF = ("ddn_api.cpp", "if (b->lpf_cap < need) { HIP_DRV_TRY(hipStreamSynchronize(st));")
GROWS_ON_HOST = {
    "ddn_front_end_run": ("ddn_api.cpp", "if (b->dec_cap[w] < need) { HIP_DRV_TRY(hipStreamSynchronize(st));"),   # (decimation passes; IQ conditioning: _LPF)
    "ddn_fm_audio_run": _LPF,
    "ddn_p25_rx_run": ("ddn_api_rx.cpp", "if (b->filt_cap < n) { HIP_TRY(hipStreamSynchronize(st));"),
    "ddn_fsk4_rx_run": ("ddn_api_rx4.cpp", "if (b->filt_cap < n) { HIP_TRY(hipStreamSynchronize(st));"),
    "ddn_cqpsk_run": ("ddn_api_cqpsk.cpp", "if (b->work_cap < need) { HIP_TRY(hipStreamSynchronize(st));"),
    "ddn_mbe_synth_batch": ("ddn_api_mbe.cpp", "if (b->rec_frames < n_frames) { HIP_TRY(hipStreamSynchronize(st));"),
}

# {name: the longest host-side time from begin() to finish() seen in this process, where the premise was asserted}: what the delay is
# sized from; the last GPU test of tests/test_stream_order_gpu.py prints it and holds it (times the margin) against the delay
HOST_MS = {}
_hip = None
_cycles_per_ms = None
_own_streams = []


def hip():
    """the HIP runtime this process's torch already loaded"""
    global _hip
    if _hip is None:
        import torch  # noqa: F401  (loads it)
        with open("/proc/self/maps") as f:
            paths = sorted({ln.split()[-1] for ln in f if re.search(r"libamdhip64\.so", ln)})
        assert paths, "no HIP runtime is mapped into this process"
        _hip = C.CDLL(paths[0])
        _hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        _hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    return _hip


def stream_flags(handle):
    f = C.c_uint(0xFFFF)
    assert hip().hipStreamGetFlags(C.c_void_p(handle), C.byref(f)) == 0
    return f.value


def new_stream():
    """a HIP stream that does not synchronise with the null stream -> torch stream (asserted non-blocking)"""
    import torch
    s = torch.cuda.Stream()
    if not stream_flags(s.cuda_stream) & HIP_STREAM_NON_BLOCKING:
        h = C.c_void_p()
        assert hip().hipStreamCreateWithFlags(C.byref(h), HIP_STREAM_NON_BLOCKING) == 0
        _own_streams.append(h)                          # (lives as long as the process: torch only borrows it)
        s = torch.cuda.ExternalStream(h.value)
    assert s.cuda_stream != 0 and stream_flags(s.cuda_stream) & HIP_STREAM_NON_BLOCKING
    return s


def delay_cycles(ms=None):
    """torch.cuda._sleep counts device clock ticks: ticks per millisecond are measured once per process"""
    global _cycles_per_ms
    import torch
    if _cycles_per_ms is None:
        probe = 2_000_000
        torch.cuda._sleep(1000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        _cycles_per_ms = probe / max(a.elapsed_time(b), 1e-3)
    return int(_cycles_per_ms * (DELAY_MS if ms is None else ms))


class Late:
    """one stream `s` and the buffers of one case.  input() / output() / inout() before begin(); then the call(s) with `handle`;
    then finish(), which asserts the premise and queues steps 4 and 5; wait() synchronises `s`; kept(t) is what step 4 copied."""

    def __init__(self, stream=None):
        self.s = stream if stream is not None else new_stream()
        self.handle = self.s.cuda_stream
        self.ins, self.outs, self.keep = [], [], {}
        self.ev = None

    def _dev(self, a):
        import torch
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()

    def input(self, truth, decoy):
        """-> the live device buffer (bytes): holds `decoy` now, `truth` from step 2 to step 5"""
        truth, decoy = np.ascontiguousarray(truth), np.ascontiguousarray(decoy)
        assert truth.nbytes == decoy.nbytes and truth.dtype == decoy.dtype
        live, t, d = self._dev(decoy), self._dev(truth), self._dev(decoy)
        self.ins.append((live, t, d))
        return live

    def output(self, nbytes):
        """-> a device buffer of marker bytes, copied to its keep buffer in step 4 and overwritten in step 5"""
        import torch
        o = torch.full((max(int(nbytes), 1),), MARKER, dtype=torch.uint8, device="cuda")
        self._out(o)
        return o

    def _out(self, o):
        import torch
        self.outs.append(o)
        self.keep[o.data_ptr()] = torch.zeros_like(o)    # (made here: nothing is allocated while the producer is queued)

    def inout(self, truth, decoy):
        live = self.input(truth, decoy)
        self._out(live)
        return live

    def begin(self, ms=None, settle=True):
        """settle: wait for the device first - the uploads above ran on the null stream, which `s` does not wait for.  A second
        producer begun beside a queued one passes False (the wait would outlast the first one's delay) and settles before both."""
        import torch
        cycles = delay_cycles(ms)
        if settle:
            torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(cycles)
            self.ev = torch.cuda.Event()
            self.ev.record(self.s)
            for live, t, _ in self.ins:
                live.copy_(t, non_blocking=True)
        self.t0 = time.perf_counter()

    def pending(self):
        return not self.ev.query()

    def finish(self, name=None, premise=True):
        """the premise, unless `name` is a call that waits on the host by design (or the case is one in which it does: premise=False);
        then steps 4 and 5"""
        import torch
        late = self.pending()
        if premise and name not in BLOCKS_HOST:
            HOST_MS[name] = max(HOST_MS.get(name, 0.0), (time.perf_counter() - self.t0) * 1e3)
        with torch.cuda.stream(self.s):
            for o in self.outs:
                self.keep[o.data_ptr()].copy_(o, non_blocking=True)
            ins = {live.data_ptr() for live, _, _ in self.ins}
            for live, _, d in self.ins:
                live.copy_(d, non_blocking=True)
            for o in self.outs:
                if o.data_ptr() not in ins:
                    o.fill_(MARKER)
        if premise and (name is None or name not in BLOCKS_HOST):
            if not late:
                self.s.synchronize()                    # (no buffer of the case is given back with work in flight)
            assert late, "%s: the delay of %d ms had run out when the call returned" % (name, DELAY_MS)
        return late

    def wait(self):
        self.s.synchronize()

    def kept(self, t, dtype=np.uint8):
        return self.keep[t.data_ptr()].cpu().numpy().view(dtype)


# ---- completeness: the stream-taking exports of include/*.h ------------------------------------------------------------------------------
def stream_takers(include_dir):
    """{function: header} of every prototype with a `void* ...stream` parameter"""
    import os
    found = {}
    for fn in sorted(os.listdir(include_dir)):
        if not fn.endswith(".h"):
            continue
        with open(os.path.join(include_dir, fn), errors="replace") as f:
            src = f.read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        src = re.sub(r"//[^\n]*", " ", src)
        for m in re.finditer(r"\b([A-Za-z_]\w*)\s*\(([^;{}()]*)\)\s*;", src):
            if re.search(r"\bvoid\s*\*\s*\w*stream\w*\s*(,|$)", m.group(2).strip()):
                found[m.group(1)] = fn
    return found
