"""ddn_node_run_host as a streaming host uses it (include/ddn_node.h: "returns when ... everything is queued and the previous input
buffer may be refilled"), on all four kinds: calls back to back without a ddn_node_wait, every call's rows in a pinned buffer of its
own, and the buffer of call k - 1 overwritten with random bytes the moment call k has returned.  Random bytes are noise to every
demodulator here, so a copy that left the host late changes the symbols that call carries into the next one, bit for bit.  The
reference never streams: one chain object over all the channels (or the same node), fed from untouched memory, waited for and read
after every call.  Every comparison is np.array_equal.

The shapes are the smallest that cross every boundary, and the traffic is pinned without a GPU (the CPU oracle loop / oracle_groups +
p2seq.run_groups on the delayed rows):
  DMR, 5 rows of iq_dmr_t3_ras_cc.npz delayed by 371 c, six calls of 15000: 61-62 accepted syncs per channel, 9-11 in every call;
  P25 Phase 2, 5 rows of iq_p25p2_cc.npz delayed by 371 c, three calls of 31000: 15-16 groups per channel, 8-10 SACCH PDUs with a
  good CRC-12 on a channel that has the site's seed, none (8-10 bursts skipped as A_NOSITE instead) on a channel with seed 0."""
import ctypes as C

import numpy as np
import pytest

import ddn
import p2seq
from conftest import golden
from test_chain_gpu import _stream
from test_chain_p25p2_gpu import SEED
from test_node_gpu import _mixed_outputs, _out_set, _pinned

pytestmark = pytest.mark.gpu

UP_TO = {"records": "counts", "flags": "counts", "sync_pos": "n_sync", "group_pos": "n_groups", "info": "n_groups", "payload": "n_groups"}


def _upload(a):
    p = C.c_void_p()
    assert ddn.lib().ddn_device_alloc(a.nbytes, C.byref(p)) == 0 and ddn.lib().ddn_device_upload(p, a.ctypes.data, a.nbytes) == 0
    return p


def _rows(name, B, n_total, lo=0):
    iq = np.ascontiguousarray(golden(name)["iq"], np.uint8)
    assert lo + 371 * (B - 1) + n_total <= len(iq)
    return np.stack([iq[lo + 371 * c:lo + 371 * c + n_total] for c in range(B)])


class _Host:
    """every call's rows in a pinned buffer of its own + the poison that overwrites them"""

    def __init__(self, rows, n_call, calls):
        self.l, self.keep, self.h = ddn.lib(), [], []
        self.nbytes = rows.shape[0] * n_call * 2
        for k in range(calls):
            piece = np.ascontiguousarray(rows[:, k * n_call:(k + 1) * n_call])
            assert piece.nbytes == self.nbytes
            p = _pinned(self.l, self.nbytes, self.keep)
            C.memmove(p, piece.ctypes.data, self.nbytes)
            self.h.append(p)
        self.noise = np.random.default_rng(0x5EED).integers(0, 256, self.nbytes, dtype=np.uint8)

    def poison(self, k):
        C.memmove(self.h[k], self.noise.ctypes.data, self.nbytes)

    def free(self):
        for p in self.keep:
            self.l.ddn_host_free_pinned(p)


def _stream_calls(node, host, ks):
    """calls ks back to back, no wait; the moment call k has returned, call k - 1's buffer is overwritten (the last call's own buffer
    stays: it is the next call, or the wait, that frees it).  Then the wait."""
    for k in ks:
        node.run_host(host.h[k])
        if k >= 1:
            host.poison(k - 1)
    node.wait()


def _equal(got, want, f, n, tag):
    """the part's arrays (channels f .. f + n of the reference's); records / flags up to the counts, positions up to their number"""
    assert got.keys() == want.keys()
    for name, a in got.items():
        w = want[name][f:f + n]
        if name in UP_TO:
            lim = got[UP_TO[name]]
            for c in range(n):
                assert np.array_equal(a[c, :lim[c]], w[c, :lim[c]]), (tag, name, f + c)
        else:
            assert np.array_equal(a, w), (tag, name, f)


# ---- DDN_NODE_FSK4 ------------------------------------------------------------------------------------------------------------------
FSK4_B, FSK4_N, FSK4_CALLS = 5, 15000, 6


def _fsk4_fields(a, n):
    r = a.results()
    return {"counts": a.fetch(r.d_counts, np.int32, (n,)), "new": a.fetch(r.d_new, np.int32, (n,)),
            "n_sync": a.fetch(r.d_n_sync, np.int32, (n,)), "records": a.fetch(r.d_records10, np.uint8, (n, r.stride_symbols, 10)),
            "flags": a.fetch(r.d_flags, np.uint8, (n, r.stride_symbols)), "sync_pos": a.fetch(r.d_sync_pos, np.int32, (n, r.max_syncs))}


@pytest.fixture(scope="module")
def fsk4_ref(built):
    """-> (rows, [what one ddn_fsk4_chain over all five channels holds after call 0 .. 5 and after the flush])"""
    rows = _rows("iq_dmr_t3_ras_cc.npz", FSK4_B, FSK4_N * FSK4_CALLS)
    one = ddn.Fsk4ChainC(FSK4_B, FSK4_N, ddn.FSK4_DMR, rf_mod=2)
    want = []
    for k in range(FSK4_CALLS):
        d = _upload(np.ascontiguousarray(rows[:, k * FSK4_N:(k + 1) * FSK4_N]))
        one.run(d)
        want.append(_fsk4_fields(one, FSK4_B))
        ddn.lib().ddn_device_free(d)
    one.flush()
    want.append(_fsk4_fields(one, FSK4_B))
    one.close()
    for w in want[:FSK4_CALLS]:                      # every compared call decodes syncs on every channel
        assert w["n_sync"].min() >= 1 and w["counts"].min() > 0, w["n_sync"]
    return rows, want


def _fsk4_node():
    cfg = ddn.Fsk4ChainConfig(0, 0, 0, 0, ddn.FSK4_DMR, 2, 0, 1, 1)
    node = ddn.NodeC(FSK4_B, FSK4_N, n_devices=2, kind=ddn.NODE_FSK4, chain_cfg=cfg)
    assert [(f, n) for _, f, n in node.info] == [(0, 3), (3, 2)]
    return node


def _fsk4_check(node, want, tag):
    for p, (_, f, n) in enumerate(node.info):
        _equal(_fsk4_fields(ddn.Fsk4ChainC(n, FSK4_N, 0, handle=node.chain_object(p)), n), want, f, n, (tag, p))


def test_fsk4_node_streams_host_input(fsk4_ref):
    """two runs of three un-waited calls, the previous call's buffer poisoned after every call: what the parts hold after call 2,
    after call 5 and after the flush (the records carried over from the call before among it) equals the one-chain reference"""
    rows, want = fsk4_ref
    host, node = _Host(rows, FSK4_N, FSK4_CALLS), _fsk4_node()
    _stream_calls(node, host, (0, 1, 2))
    _fsk4_check(node, want[2], 2)
    _stream_calls(node, host, (3, 4, 5))
    _fsk4_check(node, want[5], 5)
    host.poison(5)
    node.flush()
    _fsk4_check(node, want[6], "flush")
    node.close()
    host.free()


def test_fsk4_node_reuses_its_device_input_sets(fsk4_ref):
    """four calls with host input and a wait after each: calls 2 and 3 land in the device input sets calls 0 and 1 used"""
    rows, want = fsk4_ref
    host, node = _Host(rows, FSK4_N, 4), _fsk4_node()
    for k in range(4):
        node.run_host(host.h[k])
        node.wait()
        _fsk4_check(node, want[k], k)
    node.close()
    host.free()


# ---- DDN_NODE_P25P2 -----------------------------------------------------------------------------------------------------------------
P2_SEEDS, P2_N, P2_CALLS = [SEED, 0, SEED, 0, SEED], 31000, 3


def _p2_fields(a, n):
    r = a.results()
    G = r.max_groups
    return {"counts": a.fetch(r.d_counts, np.int32, (n,)), "new": a.fetch(r.d_new, np.int32, (n,)),
            "n_groups": a.fetch(r.d_n_groups, np.int32, (n,)), "records": a.fetch(r.d_records10, np.uint8, (n, r.stride_symbols, 10)),
            "flags": a.fetch(r.d_flags, np.uint8, (n, r.stride_symbols)), "group_pos": a.fetch(r.d_group_pos, np.int32, (n, G)),
            "info": a.fetch(r.d_info, np.int32, (n, G, 4, 8)), "payload": a.fetch(r.d_payload, np.uint8, (n, G, 4, 180))}


@pytest.fixture(scope="module")
def p2_ref(built):
    """-> (rows, [what one ddn_p25p2_chain over all five channels holds after call 0 .. 2 and after the flush]); the traffic that makes
    a wrong seed visible is there: groups on every channel, SACCH PDUs with a good CRC-12 exactly on the channels that have a seed"""
    B = len(P2_SEEDS)
    rows = _rows("iq_p25p2_cc.npz", B, P2_N * P2_CALLS)
    one = ddn.P25P2ChainC(P2_SEEDS, P2_N, vocoder=0)
    want = []
    for k in range(P2_CALLS):
        d = _upload(np.ascontiguousarray(rows[:, k * P2_N:(k + 1) * P2_N]))
        one.run(d)
        want.append(_p2_fields(one, B))
        ddn.lib().ddn_device_free(d)
    one.flush()
    want.append(_p2_fields(one, B))
    one.close()
    groups, sacch, nosite = np.zeros(B, int), np.zeros(B, int), np.zeros(B, int)
    for w in want:
        for c in range(B):
            info = w["info"][c, :w["n_groups"][c]].reshape(-1, 8)
            groups[c] += int(w["n_groups"][c])
            sacch[c] += int(np.count_nonzero((info[:, 4] == p2seq.A_SACCH_S) & ((info[:, 7] & 2) != 0)))
            nosite[c] += int(np.count_nonzero(info[:, 4] == p2seq.A_NOSITE))
    assert groups.min() >= 6, groups
    for c, seed in enumerate(P2_SEEDS):
        assert (sacch[c] >= 1 and nosite[c] == 0) if seed else (sacch[c] == 0 and nosite[c] >= 1), (c, sacch, nosite)
    return rows, want


def _p2_node():
    B = len(P2_SEEDS)
    cfg = ddn.P25P2ChainConfig(0, 0, 0, 0, 0, 0, 0, 0.0)
    node = ddn.NodeC(B, P2_N, vocoder=0, n_devices=2, kind=ddn.NODE_P25P2, chain_cfg=cfg, seed44=np.array(P2_SEEDS, np.uint64))
    assert ddn.lib().ddn_node_kind_of(node.h) == ddn.NODE_P25P2
    assert [(f, n) for _, f, n in node.info] == [(0, 3), (3, 2)]      # part 1 starts on a channel without a seed
    return node


def _p2_check(node, want, tag):
    for p, (_, f, n) in enumerate(node.info):
        _equal(_p2_fields(ddn.P25P2ChainC([0] * n, P2_N, handle=node.chain_object(p)), n), want, f, n, (tag, p))


def test_p25p2_node_equals_one_chain(p2_ref):
    """kind = DDN_NODE_P25P2 with a wait after every call: every part decodes its channels with its own slice of the seed array (a
    seed-0 channel skips the scrambled bursts, a seeded one decodes their PDUs), call by call and through the flush"""
    rows, want = p2_ref
    host, node = _Host(rows, P2_N, P2_CALLS), _p2_node()
    for k in range(P2_CALLS):
        node.run_host(host.h[k])
        node.wait()
        _p2_check(node, want[k], k)
    node.flush()
    _p2_check(node, want[P2_CALLS], "flush")
    node.close()
    host.free()


def test_p25p2_node_streams_host_input(p2_ref):
    """three un-waited calls, the previous call's buffer poisoned after every call, then the wait and the flush.  (Today
    ddn_p25p2_chain_run waits for its stream in every call - the decoder lists' lengths come back to the host - so no input copy of
    this kind is ever pending when a call returns, with or without the node's own wait: this test holds the promise should that
    change, it has not been seen to fail.)"""
    rows, want = p2_ref
    host, node = _Host(rows, P2_N, P2_CALLS), _p2_node()
    _stream_calls(node, host, range(P2_CALLS))
    _p2_check(node, want[P2_CALLS - 1], P2_CALLS - 1)
    host.poison(P2_CALLS - 1)
    node.flush()
    _p2_check(node, want[P2_CALLS], "flush")
    node.close()
    host.free()


# ---- DDN_NODE_MIXED -----------------------------------------------------------------------------------------------------------------
MIX_COUNTS, MIX_N, MIX_CALLS = (5, 4, 3), 18000, 5


def _mixed_flush(m, counts):
    """what ddn_node_flush does with a part's ddn_mixed_chain, on one over all channels"""
    l = ddn.lib()
    m.wait()
    if counts[0]:
        assert l.ddn_p25_chain_flush(l.ddn_mixed_chain_part(m.h, 0)) == 0
    for g in (1, 2):
        if counts[g]:
            assert l.ddn_fsk4_chain_flush(l.ddn_mixed_chain_part(m.h, g), None) == 0


@pytest.fixture(scope="module")
def mixed_ref(built):
    """-> (rows [P25 | DMR | NXDN48], what one ddn_mixed_chain over all channels holds after the last call, and after the flush)"""
    import p25gen
    Bp, Bd, Bn = MIX_COUNTS
    n_total = MIX_N * MIX_CALLS
    rng = np.random.default_rng(21)
    dib = [np.concatenate([p25gen.make_frames(rng, 1, 0x293, crc=True, blocks=1 + (c + k) % 3)[0] for k in range(10 * MIX_CALLS)]) for c in range(Bp)]
    p25 = np.stack([p25gen.modulate_cu8(dib[c], n_total, lead=250 + 31 * c, seed=c) for c in range(Bp)])
    dmr, nx = _rows("iq_dmr_t3_ras_cc.npz", Bd, n_total), _rows("iq_nxdn48.npz", Bn, n_total, lo=60000)
    one = ddn.MixedChainC(Bp, Bd, Bn, MIX_N)
    for k in range(MIX_CALLS):
        ps = [_upload(np.ascontiguousarray(x[:, k * MIX_N:(k + 1) * MIX_N])) for x in (p25, dmr, nx)]
        one.run(*ps)
        one.wait()
        for p in ps:
            ddn.lib().ddn_device_free(p)
    last = _mixed_outputs(one.h, MIX_COUNTS, MIX_N)
    _mixed_flush(one, MIX_COUNTS)
    flushed = _mixed_outputs(one.h, MIX_COUNTS, MIX_N)
    one.close()
    assert last["p25.d_n_syncs"].min() >= 1 and last["1.d_n_sync"].min() >= 1 and last["2.d_n_sync"].min() >= 1
    return np.concatenate([p25, dmr, nx]), last, flushed


def _mixed_check(node, groups, want, tag):
    for p in range(node.parts):
        got = _mixed_outputs(node.chain_object(p), tuple(n for _, n in groups[p]), MIX_N)
        for name, a in got.items():
            g = 0 if name.startswith("p25.") else int(name[0])
            f, n = groups[p][g]
            w = want[name][f:f + n]
            if name.endswith(("d_records10", "d_flags")):
                lim = got[name.rsplit(".", 1)[0] + ".d_counts"]
            elif name.endswith("d_sync_pos"):
                lim = got["%d.d_n_sync" % g]
            elif name in ("p25.d_nid4", "p25.d_tsbk"):
                lim = got["p25.d_n_syncs"]
            else:
                assert np.array_equal(a, w), (tag, p, name)
                continue
            for c in range(n):
                assert np.array_equal(a[c, :lim[c]], w[c, :lim[c]]), (tag, p, name, c)


@pytest.mark.parametrize("overlap", [0, 1])
def test_mixed_node_streams_host_input(mixed_ref, overlap):
    """five un-waited calls (the node's own wait before it reuses an input set is taken twice), the previous call's buffer poisoned
    after every call; with the default and the overlapped schedule of the parts' chain objects"""
    rows, last, flushed = mixed_ref
    Bp, Bd, Bn = MIX_COUNTS
    host = _Host(rows, MIX_N, MIX_CALLS)
    node = ddn.NodeC(Bp, MIX_N, n_devices=3, kind=ddn.NODE_MIXED, n_dmr=Bd, n_nxdn48=Bn, overlap=overlap)
    groups = [node.groups(p) for p in range(node.parts)]
    assert node.parts == 3 and [sum(groups[p][g][1] for p in range(3)) for g in range(3)] == [Bp, Bd, Bn]
    _stream_calls(node, host, range(MIX_CALLS))
    _mixed_check(node, groups, last, MIX_CALLS - 1)
    host.poison(MIX_CALLS - 1)
    node.flush()
    _mixed_check(node, groups, flushed, "flush")
    node.close()
    host.free()


# ---- DDN_NODE_P25 -------------------------------------------------------------------------------------------------------------------
def test_p25_node_streams_host_input_and_results(built):
    """ddn_p25_chain_run_host's streaming protocol (tests/test_chain_gpu.py::test_run_host_streaming_host_never_waits) through the
    node's threads and outs[] plumbing: two pinned input buffers refilled in turn as soon as the next call has returned, three result
    sets per part used in turn, call k's read once call k + 3 has returned, no wait until the end.  Every field of every call equals a
    run of the same node that waits after every call."""
    l = ddn.lib()
    B, n_call, calls, parts = 7, 16384, 6, 3
    iq = _stream(B, n_call * calls)
    shp = ddn.P25ChainC(1, n_call)
    F, Fv, st, E = shp.F, shp.Fv, shp.stride, shp.E
    shp.close()

    def go(streaming):
        keep = []
        node = ddn.NodeC(B, n_call, n_devices=parts)
        assert node.parts == parts
        sets = [[_out_set(l, n, F, Fv, st, E, keep) for _, _, n in node.info] for _ in range(3)]
        h_in = [_pinned(l, B * n_call * 2, keep) for _ in range(2)]
        got = []

        def read(k):
            got.append([{name: a.copy() for name, a in v.items()} for _, v in sets[k % 3]])
            for _, v in sets[k % 3]:
                for a in v.values():
                    a.view(np.uint8)[...] = 0xA5              # a stale set must not pass for a result

        for k in range(calls):
            part = np.ascontiguousarray(iq[:, k * n_call:(k + 1) * n_call])
            C.memmove(h_in[k & 1], part.ctypes.data, part.nbytes)     # legal: call k - 1 (the last user of k - 2's buffer) has returned
            node.run_host(h_in[k & 1], [o for o, _ in sets[k % 3]])
            if not streaming:
                node.wait()
                read(k)
            elif k >= 3:
                read(k - 3)
        if streaming:
            node.wait()
            for k in range(calls - 3, calls):
                read(k)
        node.flush()
        node.close()
        for p in keep:
            l.ddn_host_free_pinned(p)
        return got

    want, got = go(False), go(True)
    assert len(want) == len(got) == calls
    voiced = decoded = 0
    for k in range(calls):
        for p in range(parts):
            w, v = want[k][p], got[k][p]
            for name in ("records10", "flags", "counts", "n_events", "nid4", "tsbk"):
                assert np.array_equal(v[name], w[name]), (k, p, name)
            for c in range(len(w["counts"])):
                ne = int(w["n_events"][c])
                assert np.array_equal(v["events"][c, :ne], w["events"][c, :ne]), (k, p, c)
                assert np.array_equal(v["event_data"][c, :ne], w["event_data"][c, :ne]), (k, p, c)
            assert np.array_equal(v["pcm"].view(np.uint32), w["pcm"].view(np.uint32)), (k, p)
            if k < 3:                                         # (the sets' first use: they were cleared when they were made)
                voiced += int(np.count_nonzero(w["pcm"]))
            decoded += int(w["counts"].sum())
    assert voiced > 0 and decoded > 0
