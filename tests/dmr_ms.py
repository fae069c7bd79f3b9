"""CPU restatement of the reference's MS / direct-mode path (src/protocol/dmr/dmr_ms.c) for the tests of the DMR MS stage
(include/ddn_fsk4.h, "DMR MS / direct mode").  TEST INFRASTRUCTURE - the product never imports this.

Two derivations of the same bursts, kept apart on purpose:
  read_stream()   the three reference functions read dibit by dibit from a stream position, in the reference's order - where a
                  burst lies falls out of the counts of dibits read and skipped;
  walk_call()     the stage's rule, call by call: a data or bootstrap burst in the call that lists its sync, a later burst of a unit
                  in the call whose row holds its last symbol, at p + 199 + 288 k.
tests/test_dmr_ms.py holds them against each other and against the reference's own counts (tests/golden/dmr_ms_vectors.json).
The block codes and BPTC are the oracle's decoders (tests/fec3.py, tests/bptc_small.py); a data burst's FEC-level results are
tests/dmr_data.py's, which the BS chain tests already use for dmr_data_burst_handler()."""
import numpy as np

import bptc_small
import dmr_data
import fec3
import rx4

LOCK = [264, 1704, 12, 0]                     # lock_symbols with the feature on
DATA_PATS, VOICE_PATS = (2, 4, 5), (3, 6, 7)  # MS, direct-mode TS1, TS2
UNUSED = -(1 << 31)


def _ok(code, bits):
    got, _, ok = fec3.oracle_decode(code, np.array(bits, np.uint8)[None])
    return bool(ok[0]), got[0]


def data_fields(pat, dib144):
    """dmr_data_sync() with dmr_stereo = 1, dmr_ms_mode = 1 (dmr_data.c:117-146, 217-257) -> (status, colour code, slot)"""
    d = [int(x) & 3 for x in dib144]
    cach = [0] * 24
    for i in range(12):                        # :123-127
        cach[rx4.CACH_IL[2 * i]], cach[rx4.CACH_IL[2 * i + 1]] = d[i] >> 1, d[i] & 1
    slot = 1 if pat == 5 else 0               # :141-143 currentslot = 0; :206-207 the direct-mode TS2 data word
    if not _ok(0, cach[:7])[0]:               # :133-137
        return 1, 0xFF, slot
    st = [b for i in list(range(61, 66)) + list(range(90, 95)) for b in (d[i] >> 1, d[i] & 1)]
    ok, fixed = _ok(5, st)                     # :227-230
    if not ok:
        return 2, 0xFF, slot
    return 0, rx4.bits_int(fixed[:4]), slot   # :233-234, 246-248: state->dmr_color_code = state->color_code


def voice_fields(vc, dib144, frag):
    """one voice burst: the frames (dmr_ms.c:285-291, 352-357), the sync field (:125-137, filed under VC - 1 for VC > 1), the TACT call
    (:95-101: the first seven CACH dibits handed over as bits - their low bits decide the syndrome) and the EMB (:139-152)"""
    d = np.array([int(x) & 3 for x in dib144], np.uint8)
    fr, _, sync, _ = rx4.dmr_voice_burst_fields(d, np.zeros(144, np.uint8), 0)
    out = dict(vc=vc, frames=fr, sync48=sync.astype(np.uint8), tact_ok=0xFF, emb_ok=0xFF, emb_cc=0xFF, power=9)
    if vc > 1:
        frag[vc - 2] = sync
        out["tact_ok"] = int(_ok(0, [int(x) & 1 for x in d[:7]])[0])
        ok, emb = _ok(7, list(sync[:8]) + list(sync[40:48]))
        out["emb_ok"] = int(ok)
        if ok:
            out["emb_cc"], out["power"] = rx4.bits_int(emb[:4]), int(emb[4])
    return out


def lc_of(frag):
    """dmr_dburst_handle_emb() (dmr_dburst.c:363-394) over the fragments of VC 2..5 -> dict(in128, lc77, errs, ok, undefined)"""
    m = np.zeros((8, 16), np.uint8)
    q, burst = 0, 0
    for col in range(16):
        for row in range(8):
            m[row, col] = frag[burst][q + 8]
            q += 1
            if q >= 32:
                q, burst = 0, burst + 1
    errs, lc, row0 = bptc_small.oracle_128x77(m.reshape(-1))
    ok = int(int(np.packbits(lc[:72]).astype(np.int64).sum()) % 31 == rx4.bits_int(lc[72:77]))
    return dict(in128=m.reshape(-1).copy(), lc77=lc.copy(), errs=int(errs), ok=ok, undefined=bool(row0))


_FEC = {}


def finish_data(b):
    """dmr_data_burst_handler()'s FEC-level results of a burst dmr_data_sync() lets through (tests/dmr_data.data_burst; one answer per
    distinct burst: the batch tests send the same traffic down many channels)"""
    if b["status"] == 0 and "fec" not in b:
        key = np.asarray(b["dib"], np.uint8).tobytes() + np.asarray(b["rel"], np.uint8).tobytes()
        if key not in _FEC:
            _FEC[key] = dmr_data.data_burst(b["dib"], b["rel"])
        b["fec"] = _FEC[key]
    return b


class State:
    def __init__(self):
        self.unit, self.next, self.cc, self.dropped = 0, 5, 16, 0
        self.frag = np.zeros((5, 48), np.uint8)


def walk_call(s, dib, rel, cnt, n_new, syncs, max_data=1 << 30, max_voice=1 << 30, max_lc=1 << 30):
    """one call of the stage on one channel.  dib / rel: the row's dibits and reliabilities, cnt records of it held; syncs: the decode
    list [(p, pattern, hand-over dibits [90], hand-over reliabilities [90])] -> dict(data, voice, lc: lists of burst dicts)"""
    out = dict(data=[], voice=[], lc=[])

    def voice(start, pre, vc, d144):
        v = voice_fields(vc, d144, s.frag)
        v.update(start=start, pre=pre)
        if v["emb_ok"] == 1:
            s.cc = v["emb_cc"]
        if len(out["voice"]) < max_voice:
            out["voice"].append(v)
        else:
            s.dropped += 1
        if vc == 6:
            if len(out["lc"]) < max_lc:
                lc = lc_of(s.frag)
                lc["pos"] = start + 143
                out["lc"].append(lc)
            else:
                s.dropped += 1

    def cycle(before):
        while s.next < 5:
            start = s.unit + 199 + 288 * s.next
            if start + 143 >= cnt or start >= before or start < 0:
                break
            voice(start, -1, s.next + 2, dib[start:start + 144])
            s.next += 1

    for j, (p, pat, pre, prel) in enumerate(syncs):
        if pat < 2 or pat > 7 or p < 0 or p + 54 >= cnt:
            continue
        cycle(p)
        d144 = np.concatenate([np.asarray(pre, np.uint8) & 3, dib[p + 1:p + 55]])
        if pat in VOICE_PATS:
            voice(p - 89, j, 1, d144)
            s.unit, s.next = p, 0
            continue
        r144 = np.concatenate([np.asarray(prel, np.uint8), rel[p + 1:p + 55]])
        status, cc, slot = data_fields(pat, d144)
        if status == 0:
            s.cc = cc
        if len(out["data"]) < max_data:
            out["data"].append(dict(start=p - 89, sync=j, pat=int(pat), slot=slot, status=status, cc=cc, dib=d144, rel=r144))
        else:
            s.dropped += 1
    cycle(1 << 30)
    s.unit -= n_new
    return out


def read_stream(dib, rel, syncs):
    """dmrMSData() / dmrMSBootstrap() + dmrMS() run on a dibit stream, sync by sync, reading as the reference reads: `at` is the next dibit
    get_dibit_and_analog_signal() returns.  -> (data, voice, lc) with absolute positions, symbols read behind every sync"""
    n = len(dib)
    data, voice, lcs, read = [], [], [], []
    frag = np.zeros((5, 48), np.uint8)
    for p, pat, pre, prel in syncs:
        at = p + 1
        if pat in DATA_PATS:                                   # dmrMSData(), :420-497
            if at + 54 > n:
                break
            d144 = np.concatenate([np.asarray(pre, np.uint8) & 3, dib[at:at + 54]])              # :436-456
            r144 = np.concatenate([np.asarray(prel, np.uint8), rel[at:at + 54]])
            at += 54
            status, cc, slot = data_fields(pat, d144)         # :477 dmr_data_sync()
            data.append(dict(start=p - 89, pat=int(pat), slot=slot, status=status, cc=cc, dib=d144, rel=r144))
            at += 144 + 66                                     # :485-494
        elif pat in VOICE_PATS:                                # dmrMSBootstrap(), :384-417
            if at + 54 > n:
                break
            d144 = np.concatenate([np.asarray(pre, np.uint8) & 3, dib[at:at + 54]])              # :399-401
            at += 54
            v = voice_fields(1, d144, frag)
            v["start"] = p - 89
            voice.append(v)
            at += 144                                          # :415 skipDibit(144)
            vc = 2                                             # dmrMS(), :323-381
            while True:
                if at + 144 > n:
                    at = n + 1
                    break
                v = voice_fields(vc, dib[at:at + 144], frag)  # :349-357: 12 + 36 + 18 + 24 + 18 + 36
                v["start"] = at
                voice.append(v)
                at += 144
                if vc == 6:                                    # :367-369
                    lc = lc_of(frag)
                    lc["pos"] = at - 1
                    lcs.append(lc)
                vc += 1                                        # :236-251
                if vc > 6:
                    break
                at += 144
            if at <= n:
                at += 144 + 66                                 # :253-259
        else:
            continue
        read.append((int(p), at - (p + 1)))
    return data, voice, lcs, read


def stream_reference(w, lock=LOCK):
    """the whole stream of one channel (tests/rx4.OracleFsk4Rx.run's dict, its loop run with lock_symbols = LOCK) as one call of the
    stage -> dict(data, voice, lc) with positions relative to the stream, data bursts finished, cc, and the frames of the talk path"""
    dib = (w["rec4"][:, 0] & 3).astype(np.uint8)
    rel = (w["rec4"][:, 1] & 0xFF).astype(np.uint8)
    syncs = [(int(p), int(w["sync_pat"][k]), w["pre"][k], w["pre_rel"][k]) for k, p in enumerate(w["sync_pos"])]
    s = State()
    out = walk_call(s, dib, rel, len(dib), 0, syncs)
    for b in out["data"]:
        finish_data(b)
    out["cc"] = s.cc
    return out


_CHAIN = {}


def chain_reference(x, c, n, key="air"):
    """channel c of the cu8 batch x as a DMR chain with the feature on sees it in calls of n samples: the pinned front end call by call,
    the oracle loop with lock_symbols = LOCK over the whole stream -> stream_reference(), plus `held`: the records the loop holds after
    each call (the same loop run call by call).  One answer per (key, c, n)."""
    import chain_fsk4_stream as cs
    if (key, c, n) not in _CHAIN:
        disc = cs.front_end_disc(x[c], n, 2)
        w = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, rf_mod=2, handler=1, lock=LOCK)).run(disc, max_sync=4096)
        r = stream_reference(w)
        loop, held, k = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, rf_mod=2, handler=1, lock=LOCK)), [], 0
        for a in range(0, len(disc), n):
            k += len(loop.run(disc[a:a + n], max_sync=n // 8 + 8)["sym"])
            held.append(k)
        assert k == len(w["sym"])
        r.update(w=w, held=np.array(held, np.int64))
        _CHAIN[(key, c, n)] = r
    return _CHAIN[(key, c, n)]
