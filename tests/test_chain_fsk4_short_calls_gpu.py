"""The fsk4 chain object (ddn_fsk4_chain, include/ddn_chain.h) at calls shorter than its carry, all eight protocols: every unit of the
stream decoded once, whole, in order and equal field for field to the whole-stream CPU reference (tests/chain_fsk4_stream.py), the
outputs carried per talk path equal over the whole stream bit for bit, d_dropped_syncs 0.

Call sizes from the trait row (T = results().carry_symbols, sps = samples per symbol): below the carry sps * (T // 3) + 1 (every sync
waits through three or more calls, boundaries off the symbol edges), at the carry sps * T (the new-record count lands on T - 1, T,
T + 1: the p < n_new edge; D-STAR + 5 samples, its generated stream has no timing drift), one demodulator block 8192 (below the carry
for D-STAR and, at 20 samples per symbol, for dPMR: about 410 records against 480), and tiny 2 * sps + 1 (two or three records per
call: a sync is re-based about a hundred times, every slot array comes down to its additive margin) for DMR, NXDN48, M17 and EDACS.  Voice to PCM (DMR, NXDN48, YSF V/D modes 1 / 2 and full-rate,
dPMR), the DMR data bursts / embedded link control, and the DMR / NXDN48 groups of a mixed chain at one block under both schedules.
tests/test_chain_fsk4_short_calls_traffic.py holds the floors these streams meet on the CPU."""
import numpy as np
import pytest

import chain_fsk4_stream as cs
import ddn

pytestmark = pytest.mark.gpu


def _carry(proto, B=1):
    gpu = {"dmr": ddn.FSK4_DMR, "nxdn48": ddn.FSK4_NXDN48, "nxdn96": ddn.FSK4_NXDN96, "m17": ddn.FSK4_M17, "ysf": ddn.FSK4_YSF,
           "dpmr": ddn.FSK4_DPMR, "dstar": ddn.FSK4_DSTAR, "edacs": ddn.FSK4_EDACS}[proto]
    row = cs.ROWS[proto]
    ch = ddn.Fsk4ChainC(B, 48000, gpu, rf_mod=0 if proto in ("nxdn48", "m17", "ysf") else 2, handlers=row["handlers"], vocoder=0)
    T = int(ch.results().carry_symbols)
    ch.close()
    return T


def _sized_as_the_floors_assume(proto, n, info):
    """the decode slots the CPU floors were held against (cs.decode_slots restates the chain's sizing rule) are the chain's own"""
    assert info["max_syncs"] == cs.decode_slots(proto, n)[0], (proto, n, info["max_syncs"])


@pytest.mark.parametrize("proto,size", cs.cases())
def test_short_calls_decode_every_unit_once_and_whole(built, proto, size):
    T = _carry(proto)
    assert T == cs.ROWS[proto]["T"]                    # (the CPU floors were taken with the table's carry)
    n = cs.call_size(proto, size, T)
    info = cs.run_and_check(proto, "tiny" if size == "tiny" else "plain", n)
    _sized_as_the_floors_assume(proto, n, info)
    new = info["new"][:-1]
    if n < cs.ROWS[proto]["sps"] * T:                  # below, tiny, and one block for D-STAR and dPMR
        assert new.max() < T                           # every call brought fewer records than the carry holds
    if size == "at":
        assert len(set(new.reshape(-1).tolist()) & {T - 1, T, T + 1}) >= 2


@pytest.mark.parametrize("proto", cs.VOICE)
def test_short_calls_voice_to_pcm(built, proto):
    """vocoder = 1 below the carry: the frames of every talk path in air order and their PCM == the CPU vocoder over the whole stream
    (the history streams from call to call)"""
    n = cs.call_size(proto, "below", _carry(proto))
    info = cs.run_and_check(proto, "voice", n, vocoder=1)
    _sized_as_the_floors_assume(proto, n, info)
    assert info["new"][:-1].max() < info["T"]


@pytest.mark.parametrize("size", cs.HANDLER_SIZES)
def test_short_calls_dmr_data_bursts_and_embedded_lc(built, size):
    """link control, rate 3/4 confirmed / unconfirmed, every other data type and the embedded link control: a burst's decision event
    and its sync fall in different calls (the selectors read the events against the decode list and the carried list)"""
    n = cs.call_size("dmr", size, _carry("dmr"))
    _sized_as_the_floors_assume("dmr", n, cs.run_and_check("dmr", "handlers", n))


@pytest.mark.parametrize("overlap", [0, 1])
def test_mixed_chain_groups_equal_their_own_chains_at_one_block(built, overlap):
    """DMR and NXDN48 groups beside a P25 group in calls of 8192 samples, default and overlapped schedule (the odd calls' second
    discriminator buffer): after every call each group's records, counts, sync list and decode outputs == its stand-alone chain's"""
    import p25gen
    n, calls = cs.MIXED_N, cs.MIXED_CALLS
    rng = np.random.default_rng(5)
    Bp = 3
    p25 = np.stack([p25gen.modulate_cu8(np.concatenate([p25gen.make_frames(rng, 1, 0x293, crc=True, blocks=1 + (c + k) % 3)[0] for k in range(24)]),
                                        n * calls, lead=250 + 31 * c, seed=c) for c in range(Bp)])
    dmr, nx = cs.stream("dmr", "mixed"), cs.stream("nxdn48", "mixed")
    assert dmr.shape[1] == nx.shape[1] == n * calls
    l = ddn.lib()
    m = ddn.MixedChainC(Bp, dmr.shape[0], nx.shape[0], n, overlap=overlap)
    own = {1: ddn.Fsk4ChainC(dmr.shape[0], n, ddn.FSK4_DMR, rf_mod=2), 2: ddn.Fsk4ChainC(nx.shape[0], n, ddn.FSK4_NXDN48, rf_mod=0)}
    seen = {1: 0, 2: 0}
    for k in range(calls):
        ps = [cs.upload(l, np.ascontiguousarray(a[:, k * n:(k + 1) * n])) for a in (p25, dmr, nx)]
        m.run(*ps)
        m.wait()
        for which, x in ((1, dmr), (2, nx)):
            Bc = x.shape[0]
            a, b = m.part(which), own[which]
            b.run(ps[which])
            ra, rb = a.results(), b.results()
            assert (ra.stride_symbols, ra.carry_symbols, ra.max_syncs) == (rb.stride_symbols, rb.carry_symbols, rb.max_syncs)
            S, st = int(ra.max_syncs), int(ra.stride_symbols)
            assert S == cs.decode_slots({1: "dmr", 2: "nxdn48"}[which], n)[0]
            cnt, ns = a.fetch(ra.d_counts, np.int32, (Bc,)), a.fetch(ra.d_n_sync, np.int32, (Bc,))
            assert np.array_equal(cnt, b.fetch(rb.d_counts, np.int32, (Bc,))) and np.array_equal(ns, b.fetch(rb.d_n_sync, np.int32, (Bc,))), (k, which)
            assert np.array_equal(a.fetch(ra.d_new, np.int32, (Bc,)), b.fetch(rb.d_new, np.int32, (Bc,))), (k, which)
            names = [("d_records10", np.uint8, (Bc, st, 10), cnt), ("d_flags", np.uint8, (Bc, st), cnt), ("d_sync_pos", np.int32, (Bc, S), ns),
                     ("d_sync_pat", np.uint8, (Bc, S), ns), ("d_pre", np.uint8, (Bc, S, 90), ns), ("d_valid", np.uint8, (Bc, S), ns)]
            names += [("d_dmr_slot_type_ok", np.uint8, (Bc, S), ns), ("d_dmr_pdu96", np.uint8, (Bc, S, 96), ns)] if which == 1 else \
                [("d_nxdn_lich", np.uint8, (Bc, S), ns), ("d_nxdn_sacch", np.uint8, (Bc, S, 4), ns), ("d_nxdn_facch", np.uint8, (Bc, S, 2, 12), ns)]
            for name, dt, shape, upto in names:
                ga, gb = a.fetch(getattr(ra, name), dt, shape), b.fetch(getattr(rb, name), dt, shape)
                for c in range(Bc):
                    assert np.array_equal(ga[c, :upto[c]], gb[c, :upto[c]]), (k, which, name, c)
            assert not a.fetch(ra.d_dropped_syncs, np.int32, (Bc,)).any()
            seen[which] += int(ns.sum())
        for p in ps:
            l.ddn_device_free(p)
    m.close()
    for b in own.values():
        b.close()
    assert seen[1] >= 12 and seen[2] >= 6, seen
