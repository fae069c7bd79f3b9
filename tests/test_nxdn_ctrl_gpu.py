"""GPU: ddn_nxdn_ctrl_decode_batch + ddn_nxdn_ctrl_walk_batch called directly on records built from generator dibits (tests/nxdngen.py,
no receive loop) against the CPU restatement (tests/nxdn_ctrl.py), array for array.  Every output array is filled with a marker first,
on both sides: a row the device leaves alone (a kind-0 slot's frame rows, a slot behind n_sync, a msg72 nothing completed) must still
hold it.  Everything is integers: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import ddn
import nxdn_ctrl as nc
import nxdngen as gen

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """the restatement of a direct case, computed once: (arrays after decode + walk, per-slot frame dicts, the walk's inputs)"""
    if name not in _REF:
        d = gen.direct_case(name)
        B, S = d["sync_pos"].shape
        out = nc.blank(B, S)
        frames = nc.decode_batch(d["rec"], d["counts"], d["sync_pos"], d["n_sync"], out)
        sa = nc.sacch_arrays(d["rec"], d["counts"], d["sync_pos"], d["n_sync"])
        nc.walk_batch(d["n_sync"], sa, out, [nc.State() for _ in range(B)], out)
        _REF[name] = (out, frames, sa)
    return _REF[name]


class Dev:
    """device copies of host arrays, freed together"""

    def __init__(self):
        self.l, self.p = ddn.lib(), []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.l.ddn_device_alloc(max(a.nbytes, 1), C.byref(p)) == 0
        if a.nbytes:
            assert self.l.ddn_device_upload(p, a.ctypes.data, a.nbytes) == 0
        self.p.append(p)
        return p

    def down(self, p, like):
        a = np.empty_like(like)
        assert self.l.ddn_device_download(a.ctypes.data, p, a.nbytes) == 0
        return a

    def free(self):
        for p in self.p:
            self.l.ddn_device_free(p)
        self.p = []


def run_device(d, sa, state=None, dev=None):
    """one decode + walk on the device -> (the fourteen output arrays, the state pointer).  state = None: a fresh block"""
    l = ddn.lib()
    own = dev is None
    dev = dev or Dev()
    B, S = d["sync_pos"].shape
    host = nc.blank(B, S)
    ptr = {k: dev.up(v) for k, v in host.items()}
    inp = ddn.NxdnCtrlInput(B, d["rec"].shape[1], S, dev.up(d["rec"]), dev.up(d["counts"]), dev.up(d["sync_pos"]), dev.up(d["n_sync"]),
                            dev.up(sa["lich"]), dev.up(sa["valid"]), dev.up(sa["sacch"]), dev.up(sa["sacch_ok"]), dev.up(sa["sacch_hard"]),
                            dev.up(sa["sacch_hard_ok"]))
    fr = ddn.NxdnCtrlFrames(*[ptr[k] for k in nc.FRAME_ARRAYS])
    ms = ddn.NxdnCtrlMessages(*[ptr[k] for k in nc.MESSAGE_ARRAYS])
    if state is None:
        state = dev.up(np.zeros(B * l.ddn_nxdn_ctrl_state_bytes(), np.uint8))
        assert l.ddn_nxdn_ctrl_state_init(state, B, None) == 0, l.ddn_last_error()
    assert l.ddn_nxdn_ctrl_decode_batch(C.byref(inp), C.byref(fr), None) == 0, l.ddn_last_error()
    assert l.ddn_nxdn_ctrl_walk_batch(C.byref(inp), C.byref(fr), state, C.byref(ms), None) == 0, l.ddn_last_error()
    got = {k: dev.down(ptr[k], host[k]) for k in host}
    if own:
        dev.free()
    return got, state


def same(got, want, where):
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert not len(bad), (where, k, bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


@pytest.mark.parametrize("name", gen.DIRECT_CASES)
def test_decode_and_walk_equal_the_restatement(built, name):
    """1, 15, 16, 17 and 33 wanted frames per decoder (sixteen code words a workgroup), a call in which one decoder, the other or neither
    has a wanted slot, sparse masks, n_sync of 0 and of max_syncs, a slot that is not valid inside a superframe, every rule of the walk"""
    d = gen.direct_case(name)
    want, frames, sa = reference(name)
    got, _ = run_device(d, sa)
    same(got, want, name)
    kinds = want["kind"][want["kind"] != nc.FILL]
    if name.startswith("wanted_"):
        n = int(name[7:])
        assert int((kinds == 1).sum()) == n and int(((kinds == 2) | (kinds == 3)).sum()) == n
    if name == "only_cac":
        assert (kinds == 1).all() and len(kinds) == 5
    if name == "only_facch2":
        assert ((kinds == 2) | (kinds == 3)).all() and len(kinds) == 3
    if name == "only_sacch":
        assert not kinds.any() and (got["bits208"] == nc.FILL).all() and (got["crc_ok"] == nc.FILL).all()
    if name == "ragged":
        assert d["n_sync"].tolist() == [0, d["sync_pos"].shape[1], 2] and (got["pf"][0] == nc.FILL).all()
    if name == "invalid_mid":
        assert sa["valid"][0].tolist() == [1, 1, 0, 1, 1, 1] and want["msg_status"][0].tolist() == [0, 0, 0, 0, 1, 0]


def test_kind_0_slots_keep_their_rows(built):
    """the frame rows of a slot without a control frame are not written: they hold what the caller put there"""
    d = gen.direct_case("sparse")
    want, frames, sa = reference("sparse")
    got, _ = run_device(d, sa)
    none = want["kind"] == 0
    assert int(none.sum()) == 36
    for k in ("bits208", "bytes26", "crc_ok", "fallback", "ran", "sf"):
        assert (got[k][none] == nc.FILL).all(), k
    assert (got["msg72"][want["msg_status"] == 0] == nc.FILL).all()


def test_the_walk_over_three_calls_equals_one_call(built):
    """the control stream's frames in one call, and cut into three calls that share the state block: the same per-frame outputs"""
    d = gen.direct_case("superframes")
    want, frames, sa = reference("superframes")
    one, _ = run_device(d, sa)
    same(one, want, "one call")
    B, S = d["sync_pos"].shape
    dev, state, parts = Dev(), None, []
    cuts = [0, S // 3, 2 * S // 3 + 1, S]
    for a, b in zip(cuts[:-1], cuts[1:]):
        ns = np.clip(d["n_sync"] - a, 0, b - a).astype(np.int32)
        sub = dict(rec=d["rec"], counts=d["counts"], sync_pos=np.ascontiguousarray(d["sync_pos"][:, a:b]), n_sync=ns)
        got, state = run_device(sub, {k: np.ascontiguousarray(v[:, a:b]) for k, v in sa.items()}, state=state, dev=dev)
        parts.append(got)
    dev.free()
    for k in want:
        joined = np.concatenate([p[k] for p in parts], axis=1)
        assert np.array_equal(joined, want[k]), k
    assert int((want["msg_status"] == 1).sum()) >= 6 and int((want["msg_status"] == 2).sum()) >= 2
