"""EDACS (-fh / -fH / -fe / -fE) through the fsk4 chain object from cu8 I/Q: every frame decoded once, whole, equal field for field to
tests/edacs.py over the restated loop's whole stream per channel, in 48 000-sample and ragged calls; the known answer "Site ID [02][002]"
(DECODE_IQ_EDACS, tests/CMakeLists.txt:8958-8963) on every channel of a batch, each starting the capture at its own offset; generated
frames under every mode; and the configuration / mode / results-getter rules of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import ddn
import edacs
import edacsgen

pytestmark = pytest.mark.gpu

N_CALL = 48000


# the collector, the whole-stream reference and the check live in tests/chain_fsk4_stream.py (the short-call tests share them)
from chain_fsk4_stream import edacs_check_chain_channel as check_chain_channel
from chain_fsk4_stream import edacs_loop_stream as loop_stream
from chain_fsk4_stream import edacs_run_chain as run_chain


def _capture_iq():
    from conftest import golden
    return np.ascontiguousarray(golden("iq_edacs.npz")["iq"], np.uint8)


@pytest.mark.parametrize("rf_mod", [2, 0])
def test_chain_known_answer_on_a_batch(built, rf_mod):
    """eight channels, each the capture rotated by its own offset (odd channels I/Q-swapped: the +EDACS words), two 48 000-sample calls
    + flush: each equals its own restated stream frame for frame, and every channel prints "Site ID [02][002]" from BCH-good frames"""
    iq = _capture_iq()
    x = np.stack([np.roll(iq, 7919 * c, axis=0)[:, ::(-1 if c & 1 else 1)] for c in range(8)])
    units = run_chain(x, N_CALL, rf_mod)
    seams = 0
    for c in range(x.shape[0]):
        got = check_chain_channel(units[c], loop_stream(x[c], N_CALL, rf_mod))
        assert {int(g["pat"]) for g in got} == {edacs.PAT_POS if c & 1 else edacs.PAT_NEG}, c
        sites = {edacs.site_line(int(g["site6"][0])) for g in got if g["kind"] == 3 and g["frame_ok"]}
        assert sites == {"Site ID [02][002]"}, (c, sites)
        seams += sum(1 for p, _ in units[c] if p // (N_CALL // 5) != (p + edacs.FRAME) // (N_CALL // 5))
    assert seams >= 4


@pytest.mark.parametrize("mode", sorted(edacs.MODES))
def test_chain_ragged_calls_every_mode(built, mode):
    """the capture in 29 989-sample calls (every boundary somewhere else inside a frame), as sent and I/Q-swapped, under every mode (the
    rotated copy has a seam where its end meets its start: the frame across it may fail its BCH check, on the device as in the restatement)"""
    iq = _capture_iq()
    n = 29989
    L = (len(iq) // n) * n
    x = np.stack([iq[:L], np.roll(iq, 5000, axis=0)[:L, ::-1]])
    units = run_chain(x, n, mode=mode)
    for c in range(2):
        got = check_chain_channel(units[c], loop_stream(x[c], n), mode)
        assert len(got) >= 40 and sum(int(g["frame_ok"]) for g in got) >= len(got) - 1, c


@pytest.mark.parametrize("mode", sorted(edacs.MODES))
def test_chain_generated_frames(built, mode):
    """generated site-ID frames (and random second messages) of both polarities come back exactly under their mode"""
    ea, esk = edacs.MODES[mode]
    rng = np.random.default_rng(17 + 2 * ea + (esk != 0))
    B, F = 4, 40
    rows, sent = [], []
    for c in range(B):
        msgs = []
        for k in range(F):
            m1 = edacsgen.ea_site_id_msg(int(rng.integers(0, 256)), int(rng.integers(0, 128)), esk) if ea else \
                edacsgen.site_id_msg(int(rng.integers(0, 32)), int(rng.integers(0, 8)), int(rng.integers(0, 32)), esk_mask=esk)
            msgs.append((m1, int(rng.integers(0, 1 << 28))))
        signs, meta = edacsgen.stream(rng, F, c & 1, gap=(0, 40), msgs=msgs)
        rows.append(edacsgen.modulate_cu8(signs, 2 * N_CALL, lead=150 + 13 * c, seed=c))
        sent.append(meta)
    units = run_chain(np.stack(rows), N_CALL, mode=mode)
    for c in range(B):
        got = [g for _, g in units[c] if g["valid"]]
        assert len(got) == F, (c, len(got))
        for g, (m1, m2, _) in zip(got, sent[c]):
            assert g["frame_ok"] and list(g["vote40"]) == [edacs.bch(m1), edacs.bch(m2)], c
            assert list(g["msg28"]) == [m1 ^ (esk << 20), m2 ^ (esk << 20)] and g["kind"] == (4 if ea else 3), c
            want = edacs.classify(m1 ^ (esk << 20), ea, True)
            assert list(g["types"]) == want[1] and list(g["site6"]) == want[2], c


def test_chain_abi(built):
    l = ddn.lib()
    for kw in (dict(handlers=1), dict(inverted=1), dict(vocoder=1), dict(rf_mod=1)):
        args = dict(rf_mod=2, handlers=0, vocoder=0)
        args.update(kw)
        with pytest.raises(ddn.DdnError, match=r"rc=-1 ddn_fsk4_chain_create"):
            ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_EDACS, **args)
    d = ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_EDACS, rf_mod=2, handlers=0, vocoder=0)
    r = d.edacs_results()
    assert (r.ea_mode, r.esk_mask) == (0, 0) and r.max_syncs >= N_CALL // 5 // 288 + 1 and r.d_raw40 and r.d_site6 and r.d_valid
    assert d.results().carry_symbols >= 48 + edacs.FRAME
    for ea, esk in ((0, 0x20), (0, 0xFF), (2, 0), (-1, 0xA0), (1, 0xA1)):
        assert l.ddn_fsk4_chain_set_edacs_mode(d.h, ea, esk) == -1
    for ea, esk in edacs.MODES.values():
        d.set_edacs_mode(ea, esk)
        assert (d.edacs_results().ea_mode, d.edacs_results().esk_mask) == (ea, esk)
    d.close()
    other = ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_DSTAR, rf_mod=2, handlers=0, vocoder=0)
    assert l.ddn_fsk4_chain_get_edacs_results(other.h, C.byref(ddn.EdacsChainResults())) == -1    # DDN_EINVAL
    assert l.ddn_fsk4_chain_set_edacs_mode(other.h, 0, 0) == -1
    other.close()
    assert l.ddn_fsk4_chain_get_edacs_results(None, None) == -1
    rx = ddn.Fsk4Rx(2, ddn.FSK4_EDACS, rf_mod=2)
    assert l.ddn_fsk4_rx_set_handlers(rx.h, 1) == -1
    rx.close()
