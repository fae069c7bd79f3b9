"""cs16 input through the chain objects and the node driver.  The format ends at the front end, so each test runs two objects of one
configuration - one fed cs16 samples x, one fed cf32 samples widen(x) (exact, tests/cs16.py) - over a few short calls and the flush,
and asks that every result array every getter hands out is equal, floats bit for bit.  Calls are the short-call tests' sizes below
the chains' carry (tiny calls of two or three records decode nothing in a few calls), so frames straddle the call boundaries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import chain_fsk4_stream as fsk4
import chain_p25p2_stream as p2
import chain_stream
import cs16
import ddn
from conftest import golden
from test_chain_gpu import _stream, _upload
from test_chain_p25p2_short_calls_gpu import _drive as p2_drive
from test_node_gpu import _mixed_outputs, _out_set, _pinned

pytestmark = pytest.mark.gpu

FORMATS = (("cs16", ddn.IN_CS16, lambda x: x), ("cf32", ddn.IN_CF32, cs16.widen))


def equal(a, b, where=""):
    """nested dicts / lists / tuples of arrays and scalars; arrays by dtype, shape and bytes (floats bit for bit)"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            equal(a[k], b[k], "%s.%s" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), (where, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            equal(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), where
    else:
        assert a == b, (where, a, b)


def rows_of(name, offsets, n_total, lo=0):
    """a golden cu8 capture as len(offsets) channels, each starting `offset` samples later, converted to cs16"""
    iq = np.ascontiguousarray(golden(name)["iq"], np.uint8)
    assert lo + max(offsets) + n_total <= len(iq)
    return cs16.cu8_to_cs16(np.stack([iq[lo + o:lo + o + n_total] for o in offsets]))


def run_p25(x, n_call, fmt, **kw):
    """x [B][calls * n_call][2] through a ddn_p25_chain in calls + the flush -> what chain_stream.Collector gathers of every getter"""
    B = x.shape[0]
    ch = ddn.P25ChainC(B, n_call, input_format=fmt, **kw)
    col = chain_stream.Collector(ch, everything=True)
    for k in range(x.shape[1] // n_call):
        d = _upload(np.ascontiguousarray(x[:, k * n_call:(k + 1) * n_call]))
        ch.run_pipelined(d)
        ch.wait()
        col.take()
        ddn.lib().ddn_device_free(d)
    ch.flush()
    col.take()
    ch.close()
    return {k: getattr(col, k) for k in ("rec", "fl", "events", "event_data", "frames", "voice")}


def test_p25_chain_c4fm_control_channel_capture(built):
    """the reference's C4FM control-channel capture, converted, on three channels 0, 1 and 37 samples apart, in calls of 6000 samples;
    the device result carries the capture's known answer, NAC 0x140 (tests/test_cs16_oracle.py holds it on the CPU)"""
    n_call, calls = 6000, 6
    x = rows_of("iq_p25p1_c4fm_cc.npz", (0, 1, 37), n_call * calls)
    got = {name: run_p25(conv(x), n_call, fmt) for name, fmt, conv in FORMATS}
    equal(got["cs16"], got["cf32"], "p25")
    for c in range(3):
        nids = [f["nid"] for _, f in sorted(got["cs16"]["frames"][c].items())][1:]      # (the first hit is a false sync)
        assert len(nids) >= 8 and all(n[0] == 1 and n[1] == 0x140 and n[2] == 7 and n[3] == 0 for n in nids), (c, nids)
        assert sum(ok for _, f in got["cs16"]["frames"][c].items() for _, ok in f["tsbk"][:1]) >= 8


def test_p25_chain_cqpsk(built):
    """modulation = CQPSK: the cs16 instances of the channel LPF ahead of the CQPSK demodulator, calls of 3201 samples"""
    n_call, calls = 3201, 8
    x = rows_of("iq_p25p1_cqpsk_cc.npz", (0, 1, 37), n_call * calls)
    got = {name: run_p25(conv(x), n_call, fmt, block_len=8192, modulation=1) for name, fmt, conv in FORMATS}
    equal(got["cs16"], got["cf32"], "p25 cqpsk")
    assert all(len(got["cs16"]["frames"][c]) >= 3 and sum(len(r) for r in got["cs16"]["rec"][c]) > 2000 for c in range(3))


@pytest.mark.parametrize("proto", ["dmr", "nxdn48"])
def test_fsk4_chain(built, proto, monkeypatch):
    """DMR and NXDN48 (two protocols: the format ends at the front end) with handlers and vocoder on, calls below the carry"""
    n = fsk4.call_size(proto, "below", fsk4.ROWS[proto]["T"])
    calls = 24
    x = cs16.cu8_to_cs16(np.ascontiguousarray(fsk4.stream(proto, "plain")[:, :calls * n]))
    run = (lambda a: fsk4.dmr_run_chain(a, n, vocoder=1)) if proto == "dmr" else (lambda a: fsk4.nxdn_run_chain(a, n, which="nxdn48", vocoder=1))
    chain_class = ddn.Fsk4ChainC

    class Tapped(chain_class):
        """the chain the stream helpers make, in the format under test; besides what they gather (sync slots, decode outputs, voice),
        the loop's own arrays of every call: counts, new, records and flags up to the counts"""
        fmt, log = None, None

        def __init__(self, *a, **k):
            super().__init__(*a, input_format=Tapped.fmt, **k)

        def _snap(self):
            r = self.results()
            cnt = self.fetch(r.d_counts, np.int32, (self.B,))
            rec = self.fetch(r.d_records10, np.uint8, (self.B, r.stride_symbols, 10))
            fl = self.fetch(r.d_flags, np.uint8, (self.B, r.stride_symbols))
            Tapped.log.append((cnt, self.fetch(r.d_new, np.int32, (self.B,)), [rec[c, :cnt[c]].copy() for c in range(self.B)],
                               [fl[c, :cnt[c]].copy() for c in range(self.B)]))

        def run(self, *a, **k):
            super().run(*a, **k)
            self._snap()

        def flush(self, *a, **k):
            super().flush(*a, **k)
            self._snap()

    monkeypatch.setattr(ddn, "Fsk4ChainC", Tapped)
    got = {}
    for name, fmt, conv in FORMATS:
        Tapped.fmt, Tapped.log = fmt, []
        got[name] = dict(run(np.ascontiguousarray(conv(x))), loop=Tapped.log)
    monkeypatch.setattr(ddn, "Fsk4ChainC", chain_class)
    assert len(got["cs16"]["loop"]) == calls + 1 and sum(int(c[0].sum()) for c in got["cs16"]["loop"]) > 0
    equal(got["cs16"], got["cf32"], proto)
    assert sum(len(u) for u in got["cs16"]["units"]) >= 3 * 4, [len(u) for u in got["cs16"]["units"]]


def test_p25p2_chain(built):
    """B = 2 synthetic voice channels of two sites, to PCM, calls of 1999 samples"""
    sps, rate, n_call = p2.VOICE_CALLS[0]
    iq, _, _, seeds = p2.voice_case(sps, rate, n_call)
    x = cs16.cu8_to_cs16(np.ascontiguousarray(iq[:, :12 * n_call]))
    got = {}
    for name, fmt, conv in FORMATS:
        filed, G = p2_drive(seeds, np.ascontiguousarray(conv(x)), n_call, 1, name, input_format=fmt)
        got[name] = ([vars(f) for f in filed], G)
    equal(got["cs16"], got["cf32"], "p25p2")
    assert all(len(f["pos"]) >= 2 for f in got["cs16"][0]), [f["pos"] for f in got["cs16"][0]]
    assert any(len(f["pcm"][s]) and np.concatenate(f["pcm"][s]).any() for f in got["cs16"][0] for s in (0, 1))


def test_mixed_chain_segmented_front_end(built):
    """3 + 2 + 2 channels: one segmented front-end launch (the SEGS instances) reads three cs16 arrays; calls of one block"""
    counts, n, calls = (3, 2, 2), 8192, 5
    xs = (rows_of("iq_p25p1_c4fm_cc.npz", (0, 1, 37), n * calls), rows_of("iq_dmr_t3_ras_cc.npz", (0, 371), n * calls),
          rows_of("iq_nxdn48.npz", (0, 371), n * calls, lo=60000))
    l = ddn.lib()
    got = {}
    for name, fmt, conv in FORMATS:
        m = ddn.MixedChainC(*counts, n, input_format=fmt)
        per_call = []
        for k in range(calls):
            ps = [_upload(np.ascontiguousarray(conv(x[:, k * n:(k + 1) * n]))) for x in xs]
            m.run(*ps)
            m.wait()
            per_call.append(_mixed_outputs(m.h, counts, n))
            for p in ps:
                l.ddn_device_free(p)
        assert l.ddn_p25_chain_flush(l.ddn_mixed_chain_part(m.h, 0)) == 0
        for g in (1, 2):
            assert l.ddn_fsk4_chain_flush(l.ddn_mixed_chain_part(m.h, g), None) == 0
        per_call.append(_mixed_outputs(m.h, counts, n))
        m.close()
        got[name] = per_call
    equal(got["cs16"], got["cf32"], "mixed")
    last = got["cs16"][calls - 1]
    assert last["p25.d_n_syncs"].min() >= 1 and sum(c["1.d_n_sync"].sum() for c in got["cs16"]) >= 4 \
        and sum(c["2.d_n_sync"].sum() for c in got["cs16"]) >= 2


def test_node_run_host_streams_cs16(built):
    """ddn_node_run_host on the P25 kind, two parts: three calls back to back from two pinned buffers, the buffer of call k - 1
    overwritten with noise the moment call k has returned (the contract of include/ddn_node.h).  Every field of every call equals the
    cf32 node's - a node that sized a cs16 sample as anything but 4 bytes would copy another stretch of the buffer"""
    l = ddn.lib()
    B, n_call, calls, parts = 5, 16384, 3, 2
    x = cs16.cu8_to_cs16(_stream(B, n_call * calls))
    shp = ddn.P25ChainC(1, n_call)
    F, Fv, st, E = shp.F, shp.Fv, shp.stride, shp.E
    shp.close()

    def go(fmt, data):
        keep = []
        node = ddn.NodeC(B, n_call, n_devices=parts, input_format=fmt)
        assert node.parts == parts
        sets = [[_out_set(l, n, F, Fv, st, E, keep) for _, _, n in node.info] for _ in range(calls)]
        nbytes = B * n_call * 2 * data.dtype.itemsize
        assert nbytes == B * n_call * l.ddn_input_format_bytes(fmt)
        h_in = [_pinned(l, nbytes, keep) for _ in range(2)]
        noise = np.random.default_rng(0x5EED).integers(0, 256, nbytes, dtype=np.uint8)
        for k in range(calls):
            part = np.ascontiguousarray(data[:, k * n_call:(k + 1) * n_call])
            assert part.nbytes == nbytes
            C.memmove(h_in[k & 1], part.ctypes.data, nbytes)
            node.run_host(h_in[k & 1], [o for o, _ in sets[k]])
            if k >= 1:
                C.memmove(h_in[(k - 1) & 1], noise.ctypes.data, nbytes)
        node.wait()
        got = [[{name: a.copy() for name, a in v.items()} for _, v in sets[k]] for k in range(calls)]
        node.flush()
        node.close()
        for p in keep:
            l.ddn_host_free_pinned(p)
        return got

    got = {name: go(fmt, np.ascontiguousarray(conv(x))) for name, fmt, conv in FORMATS}
    equal(got["cs16"], got["cf32"], "node")
    assert sum(int(v["counts"].sum()) for call in got["cs16"] for v in call) > 0
    assert sum(int(np.count_nonzero(v["pcm"])) for call in got["cs16"] for v in call) > 0


def test_decode_capture_tool_reads_a_cs16_capture(built, tmp_path, capsys):
    """tools/decode_capture.py on the control-channel capture as cu8 and converted to cs16 (sidecar sample_format "cs16", endianness
    "little"): the same frame lines; a difference is reported line by line"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import decode_capture
    u8 = np.ascontiguousarray(golden("iq_p25p1_c4fm_cc.npz")["iq"], np.uint8)
    p8 = cs16.write_capture(str(tmp_path / "cc_cu8.iq"), u8, "cu8")
    p16 = cs16.write_capture(str(tmp_path / "cc_cs16.iq"), cs16.cu8_to_cs16(u8), "cs16")
    head = []
    a = decode_capture.decode(p8, lock=336, out=head.append)
    b = decode_capture.decode(p16, lock=336, out=head.append)
    assert any("cs16 @ 48000 Hz" in h for h in head) and any("cu8 @ 48000 Hz" in h for h in head), head[:2]
    differ = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert len(a) == len(b) and not differ, "lines that differ (cu8, cs16): %s" % (differ[:10],)
    assert len(a) >= 24 and sum("NAC 140" in t for t in a) >= 24
