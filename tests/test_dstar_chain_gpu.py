"""D-STAR (-fd) through the fsk4 chain object from cu8 I/Q: every unit decoded once, whole, equal field for field to tests/dstar.py's
decode_stream() over the oracle's whole stream per channel, in 48 000-sample and ragged 29 989-sample calls, on delayed and negated copies
of the reference's capture; the known answer "SRC: KB7WUK" (DECODE_IQ_DSTAR, tests/CMakeLists.txt:8951) read through
ddn_fsk4_chain_get_dstar_results; and the configuration / results-getter rules of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import ddn
import dstar
import rx4

pytestmark = pytest.mark.gpu

N_CALL = 48000


# the collector, the whole-stream reference and the check live in tests/chain_fsk4_stream.py (the short-call tests share them)
from chain_fsk4_stream import dstar_check_chain_channel as check_chain_channel
from chain_fsk4_stream import dstar_oracle_stream as oracle_stream
from chain_fsk4_stream import dstar_run_chain as run_chain


def src_of(got):
    return [bytes(g["sh41"][27:39]).decode("latin-1") for _, g in got if g["kind"] == dstar.SD_HEADER and g["sok"]]


def _capture_iq():
    from conftest import golden
    return np.ascontiguousarray(golden("iq_dstar.npz")["iq"], np.uint8)


def _delay(iq, d, rng):
    out = np.empty_like(iq)
    out[:d] = np.clip(np.rint(127.5 + rng.normal(0, 3, (d, 2))), 0, 255).astype(np.uint8)
    out[d:] = iq[:len(iq) - d]
    return out


@pytest.mark.parametrize("rf_mod", [2, 0])
def test_chain_known_answer_on_a_batch(built, rf_mod):
    """four channels (the capture; delayed by 12345 and by 30000 samples; negated - I/Q swapped, the negative words), 48 000-sample calls
    + flush: each equals its own oracle stream unit for unit, and every channel reads SRC: KB7WUK from the slow data"""
    iq = _capture_iq()
    rng = np.random.default_rng(9)
    x = np.stack([iq, _delay(iq, 12345, rng), _delay(iq, 30000, rng), iq[:, ::-1]])
    units = run_chain(x, N_CALL, rf_mod)
    seams = 0
    for c in range(x.shape[0]):
        want = oracle_stream(x[c], N_CALL, rf_mod)
        got = check_chain_channel(units[c], want)
        pats = {int(g["pat"]) for _, g in got}
        assert pats & ({dstar.PAT_VOICE_NEG, dstar.PAT_HD_NEG} if c == 3 else {dstar.PAT_VOICE_POS, dstar.PAT_HD_POS}), (c, pats)
        srcs = src_of(got)
        assert srcs and all(s.startswith("KB7WUK") for s in srcs), (c, srcs)
        # units that straddle a call boundary (a call = N_CALL / 10 symbols at 4800 symbols/s)
        seams += sum(1 for p, g in got if (p // (N_CALL // 10)) != ((p + dstar.unit_len(int(g["pat"]))) // (N_CALL // 10)))
    assert seams >= 4


def test_chain_ragged_calls(built):
    """the capture in 29 989-sample calls (every boundary somewhere else inside a unit): as sent, rotated by 5000 samples, negated"""
    iq = _capture_iq()
    n = 29989
    L = (len(iq) // n) * n
    x = np.stack([iq[:L], np.roll(iq, 5000, axis=0)[:L], iq[:L, ::-1]])
    units = run_chain(x, n)
    for c in range(3):
        got = check_chain_channel(units[c], oracle_stream(x[c], n))
        assert len(got) >= 3, (c, len(got))
        srcs = src_of(got)
        assert srcs and all(s.startswith("KB7WUK") for s in srcs), (c, srcs)


def test_chain_abi(built):
    l = ddn.lib()
    assert hasattr(l, "ddn_fsk4_chain_get_dstar_results")
    for kw in (dict(handlers=1), dict(inverted=1), dict(vocoder=1), dict(rf_mod=1)):
        args = dict(rf_mod=2, handlers=0, vocoder=0)
        args.update(kw)
        with pytest.raises(ddn.DdnError, match=r"rc=-1 ddn_fsk4_chain_create"):
            ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_DSTAR, **args)
    d = ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_DSTAR, rf_mod=2, handlers=0, vocoder=0)
    r = d.dstar_results()
    assert r.max_syncs >= N_CALL // 10 // 2016 + 1 and r.d_hdr41 and r.d_sd_text and r.d_valid
    assert d.results().carry_symbols >= dstar.HEADER_SYMS + dstar.VOICE_SYMS
    d.close()
    other = ddn.Fsk4ChainC(2, N_CALL, ddn.FSK4_DPMR, rf_mod=2, handlers=0, vocoder=0)
    assert l.ddn_fsk4_chain_get_dstar_results(other.h, C.byref(ddn.DstarChainResults())) == -1    # DDN_EINVAL
    other.close()
    assert l.ddn_fsk4_chain_get_dstar_results(None, None) == -1
