"""D-STAR (-fd) through the fsk4 chain object from cu8 I/Q: every unit decoded once, whole, equal field for field to tests/dstar.py's
decode_stream() over the oracle's whole stream per channel, in 48 000-sample and ragged 29 989-sample calls, on delayed and negated copies
of the reference's capture; the known answer "SRC: KB7WUK" (DECODE_IQ_DSTAR, tests/CMakeLists.txt:8951) read through
ddn_fsk4_chain_get_dstar_results; and the configuration / results-getter rules of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import ddn
import dstar
import orc
import rx4

pytestmark = pytest.mark.gpu

N_CALL = 48000


def _upload(l, part):
    p = C.c_void_p()
    assert l.ddn_device_alloc(part.nbytes, C.byref(p)) == 0 and l.ddn_device_upload(p, part.ctypes.data, part.nbytes) == 0
    return p


def run_chain(x, n, rf_mod=2):
    """x: cu8 [B][samples][2] in calls of n samples + flush -> per channel [(absolute sync position, pattern, slot outputs)]"""
    l = ddn.lib()
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DSTAR, rf_mod=rf_mod, handlers=0, vocoder=0)
    units = [[] for _ in range(B)]
    base = np.zeros(B, np.int64)

    def take():
        r, rd = ch.results(), ch.dstar_results()
        S, T = rd.max_syncs, r.carry_symbols
        f = ch.fetch
        pos, new, ns = f(rd.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,)), f(rd.d_n_sync, np.int32, (B,))
        got = dict(pat=f(rd.d_sync_pat, np.uint8, (B, S)), thr=f(rd.d_sync_thr5, np.float32, (B, S, 5)), h41=f(rd.d_hdr41, np.uint8, (B, S, 41)),
                   hok=f(rd.d_hdr_crc_ok, np.uint8, (B, S)), hv=f(rd.d_hdr_valid, np.uint8, (B, S)),
                   ambe=f(rd.d_ambe_fr, np.uint8, (B, S, 21, 4, 24)), sdb=f(rd.d_sd_bytes, np.uint8, (B, S, 60)),
                   kind=f(rd.d_sd_kind, np.uint8, (B, S)), sh41=f(rd.d_sd_hdr41, np.uint8, (B, S, 41)), sok=f(rd.d_sd_crc_ok, np.uint8, (B, S)),
                   text=f(rd.d_sd_text, np.uint8, (B, S, 60)), valid=f(rd.d_valid, np.uint8, (B, S)))
        for c in range(B):
            for k in range(int(ns[c])):
                units[c].append((int(base[c]) + int(pos[c, k]) - int(T), {key: v[c, k] for key, v in got.items()}))
            base[c] += int(new[c])

    for k in range(x.shape[1] // n):
        p = _upload(l, np.ascontiguousarray(x[:, k * n:(k + 1) * n]))
        ch.run(p)
        take()
        l.ddn_device_free(p)
    ch.flush()
    take()
    ch.close()
    return units


def oracle_stream(xc, n, rf_mod=2):
    """one channel through the pinned front end (6.25 kHz filter, call by call as the chain) and the oracle loop -> (syncs, patterns,
    decode_stream)"""
    fe = orc.OracleFrontEnd(profile=1)
    calls = len(xc) // n
    disc = np.concatenate([fe.run_cu8(np.ascontiguousarray(xc[k * n:(k + 1) * n]), 8192) for k in range(calls)])
    o = rx4.OracleFsk4Rx(dstar.profile(rf_mod)).run(disc, max_sync=4096)
    return o, dstar.decode_stream(o["sym"], o["sync_pos"], o["sync_pat"], o["sync_thr"])


def check_chain_channel(units_c, want):
    """every unit of the oracle's stream, once, in order, equal field for field"""
    o, dec = want
    assert len({p for p, _ in units_c}) == len(units_c), "a unit decoded twice"
    got = [(p, g) for p, g in units_c if g["valid"]]
    assert [p for p, _ in got] == [int(o["sync_pos"][k]) for k, _ in dec], (len(got), len(dec))
    for (p, g), (k, u) in zip(got, dec):
        assert int(g["pat"]) == u["pat"] and np.array_equal(g["thr"].view(np.uint32), o["sync_thr"][k].view(np.uint32)), k
        if u["pat"] >= 2:
            assert g["hv"] and bytes(g["h41"]) == bytes(u["header41"]) and bool(g["hok"]) == bool(u["header_crc_ok"]), k
        else:
            assert not g["hv"] and not g["h41"].any()
        sd = u["sd"]
        assert np.array_equal(g["ambe"], u["ambe"]), k
        assert bytes(g["sdb"]) == sd["bytes"] and int(g["kind"]) == sd["kind"], k
        assert bytes(g["sh41"]) == sd["hdr41"] and bool(g["sok"]) == sd["crc_ok"], k
        assert bytes(g["text"]) == (sd["text"] or bytes(60)), k
    return got


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
