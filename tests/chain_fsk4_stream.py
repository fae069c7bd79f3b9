"""Stream-level collectors, whole-stream references and checks for the fsk4 chain object (ddn_fsk4_chain, include/ddn_chain.h), one
set per protocol: DMR, NXDN48 / NXDN96, M17, YSF, dPMR, D-STAR, EDACS.  TEST INFRASTRUCTURE - the product never imports this.

  collector  <proto>_run_chain: ddn.Fsk4ChainC call by call + flush; after every call each decoded unit is filed under its absolute sync
             position (base + pos - carry_symbols, base advanced by d_new), the outputs carried per talk path (voice frames, PCM, DMR
             data bursts, embedded link control, M17 LICH-reassembled LSFs) in order, d_dropped_syncs and the calls' d_new in `info`
  reference  <proto>_oracle_stream: the pinned front-end oracle call by call at the same samples_per_call (the front end's block
             schedule follows the calls), then ONE run of the oracle receive loop over the whole discriminator stream and the
             protocol's restatement over the whole symbol stream - no call boundary behind the front end
  check      <proto>_check_chain_channel: every unit of the reference once, in order, field for field (thresholds as uint32), no
             position twice; check_info: nothing dropped

The short-call tests (tests/test_chain_fsk4_short_calls_gpu.py) and their traffic floors (tests/test_chain_fsk4_short_calls_traffic.py)
build on the tables at the end: carry lengths, samples per symbol, call sizes and the input streams."""
import ctypes as C

import numpy as np

import ddn
import dpmr
import dstar
import edacs
import orc
import rx4


def upload(l, part):
    p = C.c_void_p()
    assert l.ddn_device_alloc(part.nbytes, C.byref(p)) == 0 and l.ddn_device_upload(p, part.ctypes.data, part.nbytes) == 0
    return p


def drive(ch, x, n, take, info=None):
    """x [B][samples][2] cu8 through chain `ch` in calls of n samples, then the flush; take() after each.  info (a dict) receives what
    every protocol's run has: dropped [B] (d_dropped_syncs after the flush), new [calls + 1][B] (d_new per call), T, max_syncs"""
    l = ddn.lib()
    B = x.shape[0]
    news = []

    def step():
        take()
        news.append(ch.fetch(ch.results().d_new, np.int32, (B,)))

    for k in range(x.shape[1] // n):
        p = upload(l, np.ascontiguousarray(x[:, k * n:(k + 1) * n]))
        ch.run(p)
        step()
        l.ddn_device_free(p)
    ch.flush()
    step()
    if info is not None:
        r = ch.results()
        info.update(dropped=ch.fetch(r.d_dropped_syncs, np.int32, (B,)), new=np.stack(news), T=int(r.carry_symbols), max_syncs=int(r.max_syncs))


def check_info(info):
    """d_dropped_syncs stays 0, and the flush brought no records"""
    assert not info["dropped"].any(), info["dropped"]
    assert not info["new"][-1].any()


def front_end_disc(xc, n, lpf):
    """one channel through the pinned front end, call by call as the chain makes them"""
    fe = orc.OracleFrontEnd(profile=lpf)
    return np.concatenate([fe.run_cu8(np.ascontiguousarray(xc[k * n:(k + 1) * n]), 8192) for k in range(len(xc) // n)])


def _unique(units_c):
    assert len({p for p, _ in units_c}) == len(units_c), "a unit decoded twice"


# ---- D-STAR -------------------------------------------------------------------------------------------------------------------------
def dstar_run_chain(x, n, rf_mod=2, info=None):
    """x: cu8 [B][samples][2] in calls of n samples + flush -> per channel [(absolute sync position, pattern, slot outputs)]"""
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

    drive(ch, x, n, take, info)
    ch.close()
    return units


def dstar_oracle_stream(xc, n, rf_mod=2):
    """one channel through the pinned front end (6.25 kHz filter, call by call as the chain) and the oracle loop -> (syncs, patterns,
    decode_stream)"""
    o = rx4.OracleFsk4Rx(dstar.profile(rf_mod)).run(front_end_disc(xc, n, 1), max_sync=4096)
    return o, dstar.decode_stream(o["sym"], o["sync_pos"], o["sync_pat"], o["sync_thr"])


def dstar_check_chain_channel(units_c, want):
    """every unit of the oracle's stream, once, in order, equal field for field"""
    o, dec = want
    _unique(units_c)
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


# ---- EDACS --------------------------------------------------------------------------------------------------------------------------
def edacs_run_chain(x, n, rf_mod=2, mode="-fh", info=None):
    """x: cu8 [B][samples][2] in calls of n samples + flush -> per channel [(absolute sync position, slot outputs)]"""
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_EDACS, rf_mod=rf_mod, handlers=0, vocoder=0)
    ch.set_edacs_mode(*edacs.MODES[mode])
    units = [[] for _ in range(B)]
    base = np.zeros(B, np.int64)

    def take():
        r, rd = ch.results(), ch.edacs_results()
        assert (rd.ea_mode, rd.esk_mask) == edacs.MODES[mode]
        S, T = rd.max_syncs, r.carry_symbols
        f = ch.fetch
        pos, new, ns = f(rd.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,)), f(rd.d_n_sync, np.int32, (B,))
        got = dict(pat=f(rd.d_sync_pat, np.uint8, (B, S)), thr=f(rd.d_sync_thr5, np.float32, (B, S, 5)), raw40=f(rd.d_raw40, np.uint64, (B, S, 6)),
                   vote40=f(rd.d_vote40, np.uint64, (B, S, 2)), bch_ok=f(rd.d_bch_ok, np.uint8, (B, S, 2)),
                   frame_ok=f(rd.d_frame_ok, np.uint8, (B, S)), msg28=f(rd.d_msg28, np.uint32, (B, S, 2)), kind=f(rd.d_kind, np.uint8, (B, S)),
                   types=f(rd.d_types, np.uint8, (B, S, 3)), site6=f(rd.d_site6, np.int32, (B, S, 6)), valid=f(rd.d_valid, np.uint8, (B, S)))
        for c in range(B):
            for k in range(int(ns[c])):
                units[c].append((int(base[c]) + int(pos[c, k]) - int(T), {key: v[c, k] for key, v in got.items()}))
            base[c] += int(new[c])

    drive(ch, x, n, take, info)
    ch.close()
    return units


def edacs_loop_stream(xc, n, rf_mod=2):
    """one channel through the pinned front end (ProVoice profile, call by call as the chain) and the restated loop"""
    return edacs.LoopRx(rf_mod).run(front_end_disc(xc, n, 3), max_sync=4096)


def edacs_check_chain_channel(units_c, o, mode="-fh"):
    """every frame of the restated stream, once, in order, equal field for field"""
    ea, esk = edacs.MODES[mode]
    assert len({p for p, _ in units_c}) == len(units_c), "a frame decoded twice"
    got = [(p, g) for p, g in units_c if g["valid"]]
    want = [(int(p), int(pat), t) for p, pat, t in zip(o["sync_pos"], o["sync_pat"], o["sync_thr"]) if int(p) + 1 + edacs.FRAME <= len(o["sym"])]
    assert [p for p, _ in got] == [p for p, _, _ in want], (len(got), len(want))
    for (p, g), (_, pat, t) in zip(got, want):
        assert int(g["pat"]) == pat and np.array_equal(g["thr"].view(np.uint32), t.view(np.uint32)), p
        u = edacs.decode_slot(o["sym"], p, pat, t, ea, esk)
        for key in ("raw40", "vote40", "bch_ok", "frame_ok", "msg28", "kind", "types", "site6"):
            assert np.array_equal(np.asarray(g[key]).astype(np.int64).reshape(-1), np.asarray(u[key], np.uint64).astype(np.int64).reshape(-1)), (p, key)
    return [g for _, g in got]


# ---- dPMR ---------------------------------------------------------------------------------------------------------------------------
DPMR_KIND = {None: 0, "called": 1, "calling": 2}


def dpmr_aiid(v):
    return None if int(v) < 0 else dpmr.air_interface_id(int(v))


def dpmr_check_superframe(got, c, k, sf):
    """slot (c, k) of the device outputs == the restatement's superframe dict"""
    for h in range(2):
        w = sf["cch"][h]
        assert np.array_equal(got["bits"][c, k, h], np.asarray(w["bits48"], np.uint8)), (c, k, h)
        assert got["ham"][c, k, h].tolist() == w["ham"], (c, k, h)
        assert bool(got["crc"][c, k, h]) == bool(w["crc_ok"]), (c, k, h)
        want = [w["fn"], dpmr.value(w["bits48"][2:14]), w["mode"], w["version"], w["format"], w["emergency"], w["reserved"], w["slow"]]
        assert got["fields"][c, k, h].tolist() == want, (c, k, h)
    assert int(got["id"][c, k]) == sf["id"] and int(got["color"][c, k]) == sf["color"], (c, k)


def dpmr_check_identity(got, c, k, sf):
    assert int(got["kind"][c, k]) == DPMR_KIND[sf["kind"]] and bool(got["strong"][c, k]) == sf["strong"], (c, k)
    assert dpmr_aiid(got["tg"][c, k]) == sf["tg"] and dpmr_aiid(got["src"][c, k]) == sf["src"], (c, k)


def dpmr_check_voice_slot(got, c, k, sf):
    halves = dpmr.voice_halves(sf)
    for f in range(8):
        assert np.array_equal(got["fr"][c, k, f], rx4.ambe2450_deinterleave(sf["voice"][f])[0]), (c, k, f)
    for h in range(2):
        assert bool(got["voiced"][c, k, h]) == halves[h] and bool(got["muted"][c, k, h]) == (sf["cch"][h]["version"] == 3), (c, k, h)


def dpmr_run_chain(x, n, inverted=0, vocoder=1, rf_mod=2, info=None):
    """x: cu8 [B][samples][2] in calls of n samples + flush -> per channel the decoded superframes
    [(absolute sync position, slot outputs)] and the synthesised frames [(absolute sync position, half, muted, pcm, result)]"""
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DPMR, rf_mod=rf_mod, inverted=inverted, handlers=0, vocoder=vocoder)
    sfs, voice = [[] for _ in range(B)], [[] for _ in range(B)]
    base = np.zeros(B, np.int64)
    seams = [0]

    def take():
        r, rd = ch.results(), ch.dpmr_results()
        S, T, F = rd.max_syncs, r.carry_symbols, rd.voice_frames
        f = ch.fetch
        pos, new, ns = f(rd.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,)), f(rd.d_n_sync, np.int32, (B,))
        got = dict(bits=f(rd.d_cch_bits2x48, np.uint8, (B, S, 2, 48)), ham=f(rd.d_ham_ok2x6, np.uint8, (B, S, 2, 6)),
                   crc=f(rd.d_crc_ok2, np.uint8, (B, S, 2)), fields=f(rd.d_fields2x8, np.int32, (B, S, 2, 8)), id=f(rd.d_id, np.int32, (B, S)),
                   color=f(rd.d_color, np.int32, (B, S)), valid=f(rd.d_valid, np.uint8, (B, S)), kind=f(rd.d_kind, np.uint8, (B, S)),
                   strong=f(rd.d_strong, np.uint8, (B, S)), tg=f(rd.d_tg, np.int32, (B, S)), src=f(rd.d_src, np.int32, (B, S)))
        if vocoder:
            assert F >= 8
            got.update(fr=f(rd.d_ambe_fr, np.uint8, (B, S, 8, 4, 24)), voiced=f(rd.d_voiced2, np.uint8, (B, S, 2)),
                       muted=f(rd.d_muted2, np.uint8, (B, S, 2)))
            nv, slot = f(rd.d_n_voice, np.int32, (B,)), f(rd.d_voice_slot, np.int32, (B, F))
            half, mut, skip = f(rd.d_voice_half, np.uint8, (B, F)), f(rd.d_voice_muted, np.uint8, (B, F)), f(rd.d_voice_skip, np.uint8, (B, F))
            res, pcm = f(rd.d_voice_result, np.int32, (B, F, 5)), f(rd.d_pcm, np.float32, (B, F, 160))
        else:
            assert F == 0 and rd.d_pcm is None
        for c in range(B):
            for k in range(int(ns[c])):
                one = {key: v[c, k] for key, v in got.items()}
                if pos[c, k] < T:
                    seams[0] += 1                  # a superframe whose sync came in the previous call
                sfs[c].append((int(base[c]) + int(pos[c, k]) - int(T), one))
            if vocoder:
                assert not pcm[c, nv[c]:].any() and skip[c, nv[c]:].all() and not skip[c, :nv[c]].any() and nv[c] % 4 == 0
                for j in range(int(nv[c])):
                    voice[c].append((int(base[c]) + int(pos[c, slot[c, j]]) - int(T), int(half[c, j]), int(mut[c, j]), pcm[c, j].copy(),
                                     res[c, j].copy()))
            base[c] += int(new[c])

    drive(ch, x, n, take, info)
    ch.close()
    return sfs, voice, seams[0]


def dpmr_oracle_stream(xc, n, inverted=0, rf_mod=2):
    """one channel through the pinned front end (call by call, as the chain) and the oracle loop -> (dibits, syncs, decode_stream)"""
    o = rx4.OracleFsk4Rx(dpmr.profile(inverted, rf_mod=rf_mod)).run(front_end_disc(xc, n, 1), max_sync=4096)
    dib, sp = o["rec4"][:, 0].astype(np.uint8), np.asarray(o["sync_pos"])
    return dib, sp, dpmr.decode_stream(dib, sp, inverted)


def dpmr_check_chain_channel(sfs_c, want):
    """every whole superframe of the oracle's stream, once, in order, equal field for field (slots the chain saw past the stream's end
    at flush are the restatement's skipped ones: valid = 0)"""
    got = [(p, g) for p, g in sfs_c if g["valid"]]
    assert len({p for p, _ in sfs_c}) == len(sfs_c), "a superframe decoded twice"
    assert [p for p, _ in got] == [int(s) for s in want[1][[k for k, _ in want[2]]]], (len(got), len(want[2]))
    for (p, g), (k, sf) in zip(got, want[2]):
        g1 = {key: v[None, None] for key, v in g.items()}
        dpmr_check_superframe(g1, 0, 0, sf)
        dpmr_check_identity(g1, 0, 0, sf)
        if "fr" in g:
            dpmr_check_voice_slot(g1, 0, 0, sf)
    return got


def dpmr_voice_plan(want):
    """the frames the reference synthesises over the whole stream, in air order: (sync position, half, muted, 36 dibits)"""
    plan = []
    for k, sf in want[2]:
        halves = dpmr.voice_halves(sf)
        frames, muted = dpmr.voice_plan([c["mode"] for c in sf["cch"]], [c["version"] for c in sf["cch"]])
        voiced = [h for h in range(2) if halves[h]]
        if voiced:
            assert muted == int(sf["cch"][voiced[-1]]["version"] == 3)
        for h in voiced:
            for i in range(4):
                plan.append((int(want[1][k]), h, int(sf["cch"][h]["version"] == 3), sf["voice"][4 * h + i]))
    return plan


def dpmr_check_chain_voice(voice_c, want, talk_path):
    """the synthesised frames == the voiced halves voice_plan selects, in air order; PCM and result rows == the CPU vocoder fed with
    the restated frames through the oracle frame FEC, history carried across the calls"""
    import mbe
    plan = dpmr_voice_plan(want)
    assert [(v[0], v[1], v[2]) for v in voice_c] == [(p[0], p[1], p[2]) for p in plan], (len(voice_c), len(plan))
    if not plan:
        return 0
    frames = np.stack([rx4.ambe2450_deinterleave(p[3])[0] for p in plan])
    bits, res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
    voc = mbe.OracleVocoder(ddn.MBE_AMBE, 1)
    F = len(plan)
    pcm, ro = np.zeros((1, F, 160), np.float32), np.zeros((1, F, 5), np.int32)
    bits, res = np.ascontiguousarray(bits[None]), np.ascontiguousarray(res[None])
    assert mbe._o().om_process_batch(ddn.MBE_AMBE, C.addressof(voc.tab), bits.ctypes.data, res.ctypes.data, 0, talk_path, 1, F, pcm.ctypes.data,
                                     ro.ctypes.data, C.addressof(voc.cur), C.addressof(voc.prev), C.addressof(voc.enh)) == 0
    for j, g in enumerate(voice_c):
        assert np.array_equal(g[3].view(np.uint32), pcm[0, j].view(np.uint32)), (talk_path, j, float(np.abs(g[3] - pcm[0, j]).max()))
        assert np.array_equal(g[4], ro[0, j]), (talk_path, j)
    return F


# ---- the CPU vocoder over one talk path's frames in order --------------------------------------------------------------------------
def synth_path(codec, talk_path, bits, res):
    """bits [F][49 | 88], res [F][5] (the frame decode's rows) -> (pcm [F][160], result rows [F][5]) of one talk path from a fresh history"""
    import mbe
    voc = mbe.OracleVocoder(codec, 1)
    F = len(bits)
    pcm, ro = np.zeros((1, F, 160), np.float32), np.zeros((1, F, 5), np.int32)
    b, r = np.ascontiguousarray(np.asarray(bits, np.uint8)[None]), np.ascontiguousarray(np.asarray(res, np.int32)[None])
    assert mbe._o().om_process_batch(codec, C.addressof(voc.tab), b.ctypes.data, r.ctypes.data, 0, talk_path, 1, F, pcm.ctypes.data,
                                     ro.ctypes.data, C.addressof(voc.cur), C.addressof(voc.prev), C.addressof(voc.enh)) == 0
    return pcm[0], ro[0]


def _same_pcm(got, want, where):
    assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), \
        (where, float(np.abs(np.asarray(got) - np.asarray(want)).max()))


# ---- DMR (the reference's handlers in the loop) -----------------------------------------------------------------------------------
DMR_RC_PAT = 8


def dmr_run_chain(x, n, vocoder=0, info=None):
    """-> dict(units [B], data [B], lc [2 B], voice [2 B]): the sync slots under their absolute positions, the dispatched data bursts,
    the embedded link controls and the voice bursts per talk path, each in air order over the calls"""
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_DMR, rf_mod=2, handlers=1, vocoder=vocoder)
    out = dict(units=[[] for _ in range(B)], data=[[] for _ in range(B)], lc=[[] for _ in range(2 * B)], voice=[[] for _ in range(2 * B)])
    base = np.zeros(B, np.int64)

    def take():
        r = ch.results()
        f = ch.fetch
        S, T = int(r.max_syncs), int(r.carry_symbols)
        db, lb, vb = r.dmr_data_bursts, r.dmr_emb_lcs, r.dmr_voice_bursts
        ns, pos, new = f(r.d_n_sync, np.int32, (B,)), f(r.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,))
        u = dict(pat=f(r.d_sync_pat, np.uint8, (B, S)), pre=f(r.d_pre, np.uint8, (B, S, 90)), valid=f(r.d_valid, np.uint8, (B, S)),
                 st=f(r.d_dmr_slot_type, np.uint8, (B, S, 20)), st_ok=f(r.d_dmr_slot_type_ok, np.uint8, (B, S)),
                 pdu=f(r.d_dmr_pdu96, np.uint8, (B, S, 96)), errs=f(r.d_dmr_bptc_errs, np.uint32, (B, S)))
        nd, st = f(r.d_dmr_n_data, np.int32, (B,)), f(r.d_dmr_data_start, np.int32, (B, db))
        slot, ty = f(r.d_dmr_data_slot, np.uint8, (B, db)), f(r.d_dmr_data_type, np.uint8, (B, db))
        bits, by = f(r.d_dmr_data_bits96, np.uint8, (B, db, 96)), f(r.d_dmr_data_bytes12, np.uint8, (B, db, 12))
        inf, errs = f(r.d_dmr_data_info196, np.uint8, (B, db, 196)), f(r.d_dmr_data_errs, np.uint32, (B, db))
        crc = f(r.d_dmr_data_crc, np.uint8, (B, db))
        un, co = f(r.d_dmr_r34_unconfirmed, np.uint8, (B, db, 18)), f(r.d_dmr_r34_confirmed, np.uint8, (B, db, 18))
        cc, pn = f(r.d_dmr_r34_confirmed_crc, np.uint8, (B, db)), f(r.d_dmr_r34_pool_n, np.int32, (B, db))
        pool = f(r.d_dmr_r34_pool, np.uint8, (B, db, 34, 24))
        ne, ep = f(r.d_dmr_n_emb, np.int32, (2 * B,)), f(r.d_dmr_emb_pos, np.int32, (2 * B, lb))
        lc, le, lo = f(r.d_dmr_emb_lc77, np.uint8, (2 * B, lb, 77)), f(r.d_dmr_emb_errs, np.uint32, (2 * B, lb)), f(r.d_dmr_emb_ok, np.uint8, (2 * B, lb))
        if vocoder:
            nv, vs = f(r.d_dmr_n_voice, np.int32, (2 * B,)), f(r.d_dmr_voice_start, np.int32, (2 * B, vb))
            fr = f(r.d_dmr_ambe_frames, np.uint8, (2 * B, vb, 3, 4, 24))
            vbits, pcm = f(r.d_dmr_ambe_bits, np.uint8, (2 * B, vb * 3, 49)), f(r.d_dmr_pcm, np.float32, (2 * B, vb * 3, 160))
            res, skip = f(r.d_dmr_ambe_result, np.int32, (2 * B, vb * 3, 5)), f(r.d_dmr_voice_skip, np.uint8, (2 * B, vb, 3))
        for c in range(B):
            for k in range(int(ns[c])):
                out["units"][c].append((int(base[c]) + int(pos[c, k]) - T, {key: v[c, k] for key, v in u.items()}))
            assert nd[c] <= db and np.all(st[c, nd[c]:] == -1)
            for j in range(int(nd[c])):
                out["data"][c].append(dict(pos=int(base[c]) + int(st[c, j]) - T + 143, slot=int(slot[c, j]), type=int(ty[c, j]),
                                           bits96=bits[c, j].copy(), bytes12=by[c, j].copy(), info=inf[c, j].copy(), errs=int(errs[c, j]),
                                           crc=int(crc[c, j]), unconfirmed=un[c, j].copy(), confirmed=co[c, j].copy(),
                                           confirmed_crc=int(cc[c, j]), pool=pool[c, j, :int(pn[c, j])].copy()))
        for tp in range(2 * B):
            assert ne[tp] <= lb and np.all(ep[tp, ne[tp]:] == -1)
            for j in range(int(ne[tp])):
                out["lc"][tp].append((int(base[tp // 2]) + int(ep[tp, j]) - T, lc[tp, j].copy(), int(le[tp, j]), int(lo[tp, j])))
            if vocoder:
                assert nv[tp] <= vb and np.all(skip[tp, :nv[tp]] == 0) and np.all(skip[tp, nv[tp]:] == 0xFF)
                assert not pcm[tp, 3 * nv[tp]:].any()
                for k in range(int(nv[tp])):
                    out["voice"][tp].append((int(base[tp // 2]) + int(vs[tp, k]) - T + 143, fr[tp, k].copy(), vbits[tp, 3 * k:3 * k + 3].copy(),
                                             pcm[tp, 3 * k:3 * k + 3].copy(), res[tp, 3 * k:3 * k + 3].copy()))
        base[:] += new

    drive(ch, x, n, take, info)
    ch.close()
    return out


def dmr_oracle_stream(xc, n):
    """-> dict(w: the loop's whole-stream output, data / lcs: dmr_data.stream_expectation, voice: the events that hand a burst to the
    vocoder)"""
    import dmr_data
    o = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, rf_mod=2, handler=1))
    w = o.run(front_end_disc(xc, n, 2), max_sync=4096)
    ev = o.events.rows()
    data, lcs = dmr_data.stream_expectation(w, ev)
    return dict(w=w, data=data, lcs=lcs, voice=[e for e in ev if e[1] == 6 and e[3] >= 1])


def dmr_units(want):
    """the whole bursts behind the stream's syncs: [(position, index)] (an RC sync carries none; the last may be cut)"""
    w = want["w"]
    return [(int(p), k) for k, p in enumerate(w["sync_pos"]) if int(w["sync_pat"][k]) != DMR_RC_PAT and int(p) + 54 < len(w["sym"])]


def dmr_check_chain_channel(run, c, want, vocoder=0):
    """sync slots (position, pattern, hand-over, slot type, BPTC), data bursts, embedded LCs and - vocoder = 1 - the voice of channel c"""
    import fec3
    import mbe
    w = want["w"]
    units = run["units"][c]
    _unique(units)
    assert [p for p, _ in units] == [int(p) for p in w["sync_pos"]], (len(units), len(w["sync_pos"]))
    whole = dict(dmr_units(want))
    for k, (p, g) in enumerate(units):
        assert int(g["pat"]) == int(w["sync_pat"][k]) and np.array_equal(g["pre"], w["pre"][k]), (c, p)
        assert bool(g["valid"]) == (p in whole), (c, p)
        if g["valid"]:
            st, info, _ = rx4.dmr_burst_fields(w["pre"][k] & 3, w["rec4"][p + 1:p + 55, 0] & 3, 0)
            fixed, _, ok = fec3.oracle_decode(5, st[None])
            assert bool(g["st_ok"]) == bool(ok[0]), (c, p)
            if ok[0]:
                assert np.array_equal(g["st"], fixed[0]), (c, p)
            bits, _, errs = fec3.oracle_bptc(info[None], 1)
            assert int(g["errs"]) == int(errs[0]), (c, p)
            if not fec3.oracle_bptc.undefined[0]:
                assert np.array_equal(g["pdu"], bits[0]), (c, p)
    got = run["data"][c]
    assert [g["pos"] for g in got] == [p for p, _, _ in want["data"]], (c, len(got), len(want["data"]))
    for g, (pos, slot, x) in zip(got, want["data"]):
        assert g["slot"] == slot and g["type"] == x["type"] and np.array_equal(g["info"], x["info"]), (c, pos)
        assert g["errs"] == x["errs"] and g["crc"] == x["crc"], (c, pos, g["type"], g["crc"], x["crc"])
        if not x["undefined"]:
            assert np.array_equal(g["bits96"], x["bits96"]) and np.array_equal(g["bytes12"], x["bytes12"]), (c, pos)
        if x["type"] == 8:
            assert np.array_equal(g["unconfirmed"], x["unconfirmed"]) and np.array_equal(g["confirmed"], x["confirmed"]), (c, pos)
            assert g["confirmed_crc"] == x["confirmed_crc"] and len(g["pool"]) == len(x["pool"]), (c, pos)
            for e, (b18, metric, ok9, dbsn) in zip(g["pool"], x["pool"]):
                assert int(e[:4].copy().view(np.int32)[0]) == metric and np.array_equal(e[4:22], b18) and (e[22], e[23]) == (ok9, dbsn), (c, pos)
        else:
            assert len(g["pool"]) == 0
    for slot in range(2):
        tp = 2 * c + slot
        glc = run["lc"][tp]
        assert [g[0] for g in glc] == [x[0] for x in want["lcs"][slot]], (tp, len(glc), len(want["lcs"][slot]))
        for g, (pos, lc77, e, ok, undefined) in zip(glc, want["lcs"][slot]):
            assert g[2] == e and (undefined or (np.array_equal(g[1], lc77) and g[3] == ok)), (tp, pos)
    if not vocoder:
        return
    syncs = {int(p): i for i, p in enumerate(w["sync_pos"])}
    for slot in range(2):
        tp = 2 * c + slot
        mine = [e for e in want["voice"] if e[4] == slot]
        gv = run["voice"][tp]
        assert [g[0] for g in gv] == [int(e[0]) for e in mine], (tp, len(gv), len(mine))
        if not mine:
            continue
        frames = []
        for e in mine:
            pos = int(e[0])
            dib = (w["rec4"][pos - 143:pos + 1, 0] & 3).astype(np.uint8)
            if pos - 54 in syncs:                  # the burst the sync search found: its first 90 dibits are the hand-over
                dib[:90] = w["pre"][syncs[pos - 54]] & 3
            frames.append(rx4.dmr_voice_burst_fields(dib, np.zeros(144, np.uint8), 0)[0])
        frames = np.concatenate(frames)
        bits, res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, frames)
        pcm, ro = synth_path(ddn.MBE_AMBE, tp, bits, res)
        assert np.array_equal(np.concatenate([g[1] for g in gv]), frames), tp
        assert np.array_equal(np.concatenate([g[2] for g in gv]), bits), tp
        _same_pcm(np.concatenate([g[3] for g in gv]), pcm, tp)
        assert np.array_equal(np.concatenate([g[4] for g in gv]), ro), tp


# ---- NXDN48 / NXDN96 (the LICH gate in the loop) ------------------------------------------------------------------------------------
NXDN = {"nxdn48": dict(gpu=ddn.FSK4_NXDN48, proto=rx4.PROTO_NXDN48, lpf=1, rf_mod=0), "nxdn96": dict(gpu=ddn.FSK4_NXDN96, proto=rx4.PROTO_NXDN96, lpf=2, rf_mod=2)}


def nxdn_run_chain(x, n, which="nxdn48", vocoder=0, info=None):
    """-> dict(units [B], voice [B]): the frames under their absolute sync positions; the synthesised frames per channel in air order
    (sync position, frame 0..3, parameter bits, PCM)"""
    B = x.shape[0]
    row = NXDN[which]
    ch = ddn.Fsk4ChainC(B, n, row["gpu"], rf_mod=row["rf_mod"], handlers=1, vocoder=vocoder)
    out = dict(units=[[] for _ in range(B)], voice=[[] for _ in range(B)])
    base = np.zeros(B, np.int64)

    def take():
        r = ch.results()
        f = ch.fetch
        S, T, vf = int(r.max_syncs), int(r.carry_symbols), int(r.voice_slots)
        ns, pos, new = f(r.d_n_sync, np.int32, (B,)), f(r.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,))
        u = dict(pat=f(r.d_sync_pat, np.uint8, (B, S)), pre=f(r.d_pre, np.uint8, (B, S, 90)), valid=f(r.d_valid, np.uint8, (B, S)),
                 lich=f(r.d_nxdn_lich, np.uint8, (B, S)), sacch=f(r.d_nxdn_sacch, np.uint8, (B, S, 4)), sacch_ok=f(r.d_nxdn_sacch_ok, np.uint8, (B, S)),
                 hard=f(r.d_nxdn_sacch_hard, np.uint8, (B, S, 32)), hard_ok=f(r.d_nxdn_sacch_hard_ok, np.uint8, (B, S)),
                 facch=f(r.d_nxdn_facch, np.uint8, (B, S, 2, 12)), facch_ok=f(r.d_nxdn_facch_ok, np.uint8, (B, S, 2)))
        if vocoder:
            skip, vbits = f(r.d_nxdn_voice_skip, np.uint8, (B, vf, 4)), f(r.d_nxdn_ambe_bits, np.uint8, (B, vf * 4, 49))
            pcm = f(r.d_nxdn_pcm, np.float32, (B, vf * 4, 160))
        for c in range(B):
            for k in range(int(ns[c])):
                out["units"][c].append((int(base[c]) + int(pos[c, k]) - T, {key: v[c, k] for key, v in u.items()}))
            if vocoder:
                assert np.all(skip[c, min(int(ns[c]), vf):] == 1) and not pcm[c].reshape(vf, 4, 160)[skip[c] != 0].any()
                for k in range(min(int(ns[c]), vf)):          # voice slot k = sync slot k of the call
                    for v in range(4):
                        if not skip[c, k, v]:
                            out["voice"][c].append((int(base[c]) + int(pos[c, k]) - T, v, vbits[c, 4 * k + v].copy(), pcm[c, 4 * k + v].copy()))
            base[c] += int(new[c])

    drive(ch, x, n, take, info)
    ch.close()
    return out


def nxdn_oracle_stream(xc, n, which="nxdn48"):
    """-> dict(w, frames: [(position, index, fields)] of the whole frames behind the stream's syncs)"""
    row = NXDN[which]
    w = rx4.OracleFsk4Rx(rx4.profile(row["proto"], rf_mod=row["rf_mod"], handler=1)).run(front_end_disc(xc, n, row["lpf"]), max_sync=4096)
    frames = []
    for k, p in enumerate(w["sync_pos"]):
        p = int(p)
        if p + 183 <= len(w["sym"]):
            d, rel = (w["rec4"][p + 1:p + 183, 0] & 3).astype(np.uint8), (w["rec4"][p + 1:p + 183, 1] & 0xFF).astype(np.uint8)
            frames.append((p, k, d, rel, rx4.nxdn_frame_fields(d, rel)))
    return dict(w=w, frames=frames)


def nxdn_voice_plan(want):
    """the voice frames the LICHs announce over the whole stream: [(position, frame 0..3, ambe_fr [4][24])]"""
    plan = []
    for p, k, d, rel, (lich7, par, *_rest) in want["frames"]:
        vo = rx4.nxdn_lich_voice(int(lich7)) if par else 0
        if vo:
            fr, _ = rx4.nxdn_voice_frames(d, rel)
            plan += [(p, v, fr[v]) for v in range(4) if vo == 3 or (vo == 1 and v < 2) or (vo == 2 and v >= 2)]
    return plan


def nxdn_check_chain_channel(run, c, want, vocoder=0):
    import fecgen
    import mbe
    w = want["w"]
    units = run["units"][c]
    _unique(units)
    assert [p for p, _ in units] == [int(p) for p in w["sync_pos"]], (len(units), len(w["sync_pos"]))
    whole = {p: f for p, _, _, _, f in want["frames"]}
    for k, (p, g) in enumerate(units):
        assert int(g["pat"]) == int(w["sync_pat"][k]) and np.array_equal(g["pre"], w["pre"][k]), (c, p)
        assert bool(g["valid"]) == (p in whole), (c, p)
        if not g["valid"]:
            continue
        lich7, par, ss, sr, fs, fr = whole[p]
        assert int(g["lich"]) == (int(lich7) | (0x80 if par else 0)), (c, p)
        hard = rx4.oracle_trellis_decode((ss.reshape(1, 72) >> 1), 32)[0]
        assert np.array_equal(g["hard"], hard) and bool(g["hard_ok"]) == rx4.nxdn_crc_ok(hard, 0), (c, p)
        # the soft K = 5 decodes of every whole frame (fresh path metrics per word, as the chain runs them): SACCH 36 steps -> 32 bits,
        # the two FACCH halves 96 steps -> 92 bits each, packed
        sacch = fecgen.oracle_nxdn(ss[None].copy(), sr[None].copy(), 36, 32)[0][0]
        assert np.array_equal(g["sacch"], sacch) and bool(g["sacch_ok"]) == rx4.nxdn_crc_ok(np.unpackbits(sacch)[:32], 0), (c, p)
        for h in range(2):
            facch = fecgen.oracle_nxdn(fs[h][None].copy(), fr[h][None].copy(), 96, 92)[0][0]
            assert np.array_equal(g["facch"][h], facch), (c, p, h)
            assert bool(g["facch_ok"][h]) == rx4.nxdn_crc_ok(np.unpackbits(facch)[:92], 1), (c, p, h)
    if not vocoder:
        return
    plan = nxdn_voice_plan(want)
    gv = run["voice"][c]
    assert [(g[0], g[1]) for g in gv] == [(p, v) for p, v, _ in plan], (c, len(gv), len(plan))
    if plan:
        bits, res, _ = mbe.oracle_frame_decode(ddn.MBE_AMBE, np.stack([f for _, _, f in plan]), soft=True)
        pcm, _ = synth_path(ddn.MBE_AMBE, c, bits, res)
        assert np.array_equal(np.stack([g[2] for g in gv]), bits), c
        _same_pcm(np.stack([g[3] for g in gv]), pcm, c)


# ---- M17 ----------------------------------------------------------------------------------------------------------------------------
def m17_run_chain(x, n, info=None):
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_M17, rf_mod=0, handlers=0, vocoder=0)
    units = [[] for _ in range(B)]
    base = np.zeros(B, np.int64)

    def take():
        r = ch.results()
        S, T = int(r.max_syncs), int(r.carry_symbols)
        f = ch.fetch
        ns, pos, new = f(r.d_n_sync, np.int32, (B,)), f(r.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,))
        u = dict(pat=f(r.d_sync_pat, np.uint8, (B, S)), thr=f(r.d_sync_thr5, np.float32, (B, S, 5)), lsf=f(r.d_m17_lsf30, np.uint8, (B, S, 30)),
                 lst=f(r.d_m17_lsf_status, np.uint8, (B, S)), cost=f(r.d_m17_lsf_cost, np.uint32, (B, S)), l6=f(r.d_m17_lich6, np.uint8, (B, S, 6)),
                 cnt=f(r.d_m17_lich_cnt, np.uint8, (B, S)), fp=f(r.d_m17_fn_payload18, np.uint8, (B, S, 18)), st=f(r.d_m17_str_status, np.uint8, (B, S)),
                 ll=f(r.d_m17_lich_lsf30, np.uint8, (B, S, 30)), lls=f(r.d_m17_lich_status, np.uint8, (B, S)))
        for c in range(B):
            for k in range(int(ns[c])):
                units[c].append((int(base[c]) + int(pos[c, k]) - T, {key: v[c, k] for key, v in u.items()}))
            base[c] += int(new[c])

    drive(ch, x, n, take, info)
    ch.close()
    return units


def m17_oracle_stream(xc, n):
    import m17
    w = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_M17)).run(front_end_disc(xc, n, 2), max_sync=4096)
    return w, m17.decode_stream(w)


def m17_check_chain_channel(units_c, want):
    """every sync of the stream once, in order, with its thresholds; LSF, stream frame and the LSF reassembled from the LICH chunks (the
    assembly buffer streams from call to call) equal the whole-stream decode; -> the reassembled LSFs [(position, status, 30 bytes)]"""
    w, fr = want
    _unique(units_c)
    assert [p for p, _ in units_c] == [f["pos"] for f in fr], (len(units_c), len(fr))
    lsfs = []
    for k, ((p, g), f) in enumerate(zip(units_c, fr)):
        assert int(g["pat"]) == f["pat"] and np.array_equal(g["thr"].view(np.uint32), w["sync_thr"][k].view(np.uint32)), p
        if f["kind"] == "lsf":
            assert g["lst"] == (2 if f["crc_ok"] else 1) and np.array_equal(g["lsf"], f["lsf30"]) and int(g["cost"]) == int(f["cost"]), p
        elif f["kind"] == "str":
            assert g["st"] == (2 if f["lich_err"] == 0 else 1) and np.array_equal(g["l6"], f["lich6"]) and g["cnt"] == f["cnt"], p
            if f["lich_err"] == 0:
                assert ((int(g["fp"][0]) << 8) | int(g["fp"][1])) == f["fn"] and np.array_equal(g["fp"][2:], f["payload"]), p
            if "lich_lsf30" in f:
                assert g["lls"] == (2 if f["lich_crc_ok"] else 1) and np.array_equal(g["ll"], f["lich_lsf30"]), p
                lsfs.append((p, int(g["lls"]), bytes(g["ll"])))
            else:
                assert g["lls"] == 0, p
        else:           # preamble, EOT, packet, BERT, or a frame the stream's end cut short
            assert g["lst"] == 0 and g["st"] == 0 and g["lls"] == 0, (p, f["kind"])
    return lsfs


# ---- YSF ----------------------------------------------------------------------------------------------------------------------------
def ysf_run_chain(x, n, vocoder=0, info=None):
    """-> dict(units [B], voice {"a" | "i": [B]}): the frames under their absolute sync positions; the frames through the AMBE and the
    IMBE talk path per channel in stream order (sync position, PCM [5][160], result rows, skip marks)"""
    B = x.shape[0]
    ch = ddn.Fsk4ChainC(B, n, ddn.FSK4_YSF, rf_mod=0, handlers=0, vocoder=vocoder)
    out = dict(units=[[] for _ in range(B)], voice={"a": [[] for _ in range(B)], "i": [[] for _ in range(B)]})
    base = np.zeros(B, np.int64)

    def take():
        r = ch.results()
        S, T, F = int(r.max_syncs), int(r.carry_symbols), int(r.ysf_voice_frames)
        f = ch.fetch
        ns, pos, new = f(r.d_n_sync, np.int32, (B,)), f(r.d_sync_pos, np.int32, (B, S)), f(r.d_new, np.int32, (B,))
        u = dict(f4=f(r.d_ysf_fich4, np.uint8, (B, S, 4)), st=f(r.d_ysf_fich_status, np.uint8, (B, S)), ve=f(r.d_ysf_fich_cost, np.uint32, (B, S)),
                 info=f(r.d_ysf_info2, np.uint8, (B, S, 2)), dch=f(r.d_ysf_dch40, np.uint8, (B, S, 2, 20)), dst=f(r.d_ysf_dch_status2, np.uint8, (B, S, 2)),
                 dcost=f(r.d_ysf_dch_cost2, np.uint32, (B, S, 2)), ambe=f(r.d_ysf_ambe49x5, np.uint8, (B, S, 5, 49)),
                 errs=f(r.d_ysf_errs2x5, np.uint8, (B, S, 5)), fr=f(r.d_ysf_frames184x5, np.uint8, (B, S, 5, 184)), nfr=f(r.d_ysf_n_frames, np.uint8, (B, S)))
        for c in range(B):
            for k in range(int(ns[c])):
                out["units"][c].append((int(base[c]) + int(pos[c, k]) - T, {key: v[c, k] for key, v in u.items()}))
        if vocoder:
            for key, nv_p, slot_p, skip_p, res_p, pcm_p in (("a", r.d_ysf_n_voice, r.d_ysf_voice_slot, r.d_ysf_voice_skip, r.d_ysf_voice_result, r.d_ysf_pcm),
                                                            ("i", r.d_ysf_imbe_n_voice, r.d_ysf_imbe_voice_slot, r.d_ysf_imbe_voice_skip,
                                                             r.d_ysf_imbe_voice_result, r.d_ysf_imbe_pcm)):
                nv, slot, skip = f(nv_p, np.int32, (B,)), f(slot_p, np.int32, (B, F)), f(skip_p, np.uint8, (B, F * 5))
                res, pcm = f(res_p, np.int32, (B, F * 5, 5)), f(pcm_p, np.float32, (B, F * 5, 160))
                for c in range(B):
                    assert nv[c] <= F and not pcm[c, 5 * nv[c]:].any() and skip[c, 5 * nv[c]:].all()
                    for j in range(int(nv[c])):
                        out["voice"][key][c].append((int(base[c]) + int(pos[c, slot[c, j]]) - T, pcm[c, 5 * j:5 * j + 5].copy(),
                                                     res[c, 5 * j:5 * j + 5].copy(), skip[c, 5 * j:5 * j + 5].copy()))
        base[:] += new

    drive(ch, x, n, take, info)
    ch.close()
    return out


def ysf_oracle_stream(xc, n):
    import ysf
    w = rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_YSF)).run(front_end_disc(xc, n, 2), max_sync=4096)
    return w, ysf.decode_frames(w), ysf.decode_payloads(w)[0]


def ysf_payload_equal(g, want, where):
    """one slot's payload outputs == ysf.decode_payloads' frame (the frame type carried from the last good FICH)"""
    pl = want["payload"]
    flags = want["fi"] | (want["dt"] << 2) | (16 if want["err"] != 0 else 0) | 32 | (128 if (pl is not None and pl["csd3"]) else 0)
    assert int(g["info"][1]) == flags, (where, int(g["info"][1]), flags)
    if pl is None:
        assert int(g["info"][0]) == 0, where
        return
    assert int(g["info"][0]) == pl["kind"], (where, int(g["info"][0]), pl["kind"])
    assert np.array_equal(g["dst"], pl["dch_status"]) and np.array_equal(g["dcost"], pl["dch_cost"]), where
    assert np.array_equal(g["dch"], pl["dch"]), where
    if pl["kind"] == 2:
        assert np.array_equal(g["ambe"], pl["ambe_d"]) and np.array_equal(g["errs"], pl["errs2"]), where
    assert int(g["nfr"]) == pl["n_frames"] and np.array_equal(g["fr"], pl["frames"]), where


def ysf_voice_plan(want):
    """-> {"a": frames through the AMBE talk path, "i": through the IMBE one}: [(position, n frames, parameter bits, frame-decode rows)]"""
    import mbe
    plan = {"a": [], "i": []}
    for f in want[2]:
        pl = f["payload"]
        if pl is None or pl["kind"] not in (1, 2, 4):
            continue
        if pl["kind"] == 2:
            ri = np.zeros((5, 5), np.int32)
            ri[:, 3] = ri[:, 4] = pl["errs2"]
            plan["a"].append((f["pos"], 5, pl["ambe_d"], ri))
        else:
            codec, shape = (ddn.MBE_AMBE, (4, 24)) if pl["kind"] == 1 else (ddn.MBE_IMBE, (8, 23))
            nf = pl["n_frames"]
            frames = np.ascontiguousarray(pl["frames"][:nf, :shape[0] * shape[1]].reshape(nf, *shape))
            bits, ri, _ = mbe.oracle_frame_decode(codec, frames)
            plan["a" if pl["kind"] == 1 else "i"].append((f["pos"], nf, bits, ri))
    return plan


def ysf_check_chain_channel(run, c, want, vocoder=0):
    w, fich, frames = want
    units = run["units"][c]
    _unique(units)
    mine = [(p, g) for p, g in units if g["st"] != 0]
    assert [p for p, _ in mine] == [f["pos"] for f in fich] == [f["pos"] for f in frames], (c, len(mine), len(fich))
    assert all(not g["info"].any() for p, g in units if g["st"] == 0)
    for (p, g), f, fr in zip(mine, fich, frames):
        assert g["st"] == {0: 1, -1: 2, -2: 3}[f["err"]] and np.array_equal(np.unpackbits(g["f4"]), f["bits"]) and int(g["ve"]) == f["cost"], (c, p)
        ysf_payload_equal(g, fr, (c, p))
    if not vocoder:
        return
    plan = ysf_voice_plan(want)
    for key, codec in (("a", ddn.MBE_AMBE), ("i", ddn.MBE_IMBE)):
        gv = run["voice"][key][c]
        assert [g[0] for g in gv] == [p[0] for p in plan[key]], (key, c, len(gv), len(plan[key]))
        if not gv:
            continue
        pcm, ro = synth_path(codec, c, np.concatenate([p[2] for p in plan[key]]), np.concatenate([p[3] for p in plan[key]]))
        at = 0
        for g, (pos, nf, _, _) in zip(gv, plan[key]):
            assert list(g[3]) == [0] * nf + [1] * (5 - nf), (key, c, pos)
            _same_pcm(g[1][:nf], pcm[at:at + nf], (key, c, pos))
            assert not g[1][nf:].any() and np.array_equal(g[2][:nf], ro[at:at + nf]), (key, c, pos)
            at += nf


# ---- generated traffic (tests/test_chain_mixed_gpu.py and tests/test_dpmr_chain_gpu.py build their streams from these too) ------------
def dmr_data_stream(rng):
    """a BS stream of data bursts (both time slots alternating): CSBKs until the colour-code gate locks, then every data type the
    handler treats differently -> (dibits, [(type, kwargs, what was sent)])"""
    import dmrgen
    plan = [(3, {})] * 8 + [(6, {}), (8, {}), (8, {}), (8, dict(confirmed=True, dbsn=0)), (8, dict(confirmed=True, dbsn=1)),
                            (8, dict(confirmed=True, dbsn=2, good_crc=False)), (7, {}), (7, dict(confirmed=True, dbsn=3)),
                            (10, dict(confirmed=True)), (1, {}), (2, {}), (1, dict(hurt=True)), (3, dict(good_crc=False)), (0, {}), (11, {}),
                            (4, {}), (5, {}), (9, {}), (6, dict(good_crc=False)), (3, {})]
    plan = plan + plan[8:]
    out, sent = [], []
    for k, (ty, kw) in enumerate(plan):
        kw = dict(kw)
        hurt = kw.pop("hurt", False)
        if ty == 8:
            s = dmrgen.r34_bytes(rng, **kw)
            info = dmrgen.r34_info(s)
        elif ty == 10:
            info = rng.integers(0, 2, 196).astype(np.uint8)
            info[96:100] = 0
            c = dmrgen.crc9_confirmed_rate1(info)
            info[7:16] = [(c >> (8 - i)) & 1 for i in range(9)]
            s = info.copy()
        else:
            s = dmrgen.payload_bits(ty, rng, **kw)
            t = s.copy()
            if hurt:
                t[16:24] ^= np.unpackbits(np.array([0xA5], np.uint8))          # one wrong byte: RS(12,9) repairs it
            info = dmrgen.bptc_196x96(t)
        out.append(dmrgen.burst(k & 1, 7, ty, info))
        sent.append((ty, kw, hurt, s))
    return np.concatenate(out), sent


def dmr_voice_stream(rng, n_superframes=4):
    """CSBKs on both slots until the colour-code gate locks, then voice superframes on slot 1 (link control embedded in bursts B..E,
    the third one with a wrong checksum) beside idle data bursts on slot 2 -> (dibits, the link controls sent)"""
    import dmrgen
    out = [dmrgen.burst(k & 1, 7, 3, dmrgen.bptc_196x96(dmrgen.payload_bits(3, rng))) for k in range(8)]
    lcs = []
    for q in range(n_superframes):
        lc = rng.integers(0, 2, 72).astype(np.uint8)
        good = q != 2
        crc5 = None if good else (int(np.packbits(lc).astype(np.int64).sum()) % 31) ^ 0x0A
        lcs.append((lc, good))
        for b in dmrgen.voice_superframe(0, 7, lc, rng, crc5):
            out += [b, dmrgen.burst(1, 7, 9, dmrgen.bptc_196x96(rng.integers(0, 2, 96)))]
    return np.concatenate(out), lcs


def dpmr_voice_transmission(rng, plan):
    """generated superframes: (mode0, mode1, version0, version1) per superframe; AMBE frames from mbe.ambe_encode"""
    import dpmrgen
    import mbe
    sfs = []
    for i, (m0, m1, v0, v1) in enumerate(plan):
        fn = (0, 1) if i % 2 == 0 else (2, 3)
        cch = [dpmrgen.cch_dibits(dpmrgen.cch_bits(fn=fn[h], half=(0x5A5, 0x3C3)[h] + i % 2, mode=(m0, m1)[h], version=(v0, v1)[h]))
               for h in range(2)]
        tch = [dpmrgen.ambe_dibits(mbe.ambe_encode(b)) for b in mbe.random_ambe_bits(rng, (8,))]
        sfs.append(dpmrgen.superframe(cch[0], cch[1], dpmrgen.color_pattern(i % 64), tch))
    return sfs


DPMR_VOICE_PLAN = [(0, 0, 0, 0), (1, 1, 0, 0), (5, 5, 0, 3), (2, 2, 0, 0), (0, 7, 3, 0), (4, 1, 0, 3), (5, 0, 3, 3), (0, 0, 0, 0)] * 3


# ---- the short-call cases ---------------------------------------------------------------------------------------------------------
# sps = 48000 / symbol rate; T = the trait row's carry (the GPU test checks it against results().carry_symbols); gap = the loop's least
# distance between two accepted syncs (0: a sync word length, the general bound); win = symbols of the sync word
ROWS = {
    "dmr": dict(sps=10, T=256, gap=0, win=24, handlers=1),
    "nxdn48": dict(sps=20, T=256, gap=0, win=10, handlers=1),
    "nxdn96": dict(sps=10, T=256, gap=0, win=10, handlers=1),
    "m17": dict(sps=10, T=256, gap=0, win=8, handlers=0),
    "ysf": dict(sps=10, T=480, gap=0, win=20, handlers=0),
    "dpmr": dict(sps=20, T=480, gap=384, win=12, handlers=0),
    "dstar": dict(sps=10, T=2688, gap=2016, win=24, handlers=0),
    "edacs": dict(sps=5, T=320, gap=288, win=48, handlers=0),
}
TINY = ("dmr", "nxdn48", "m17", "edacs")          # units under 500 symbols
SIZES = ("below", "at", "block", "tiny")
# the at-the-carry size moved by a few samples where sps * T alone gave one new-record count on the protocol's stream
AT_SHIFT = {"dstar": 5}   # (the generated D-STAR stream has no timing drift: every call of 26 880 samples brought 2688 records)


def call_size(proto, size, T=None):
    row = ROWS[proto]
    T = row["T"] if T is None else T
    return {"below": row["sps"] * (T // 3) + 1, "at": row["sps"] * T + AT_SHIFT.get(proto, 0), "block": 8192, "tiny": 2 * row["sps"] + 1}[size]


def decode_slots(proto, n):
    """the chain's decode slots per channel and call (fsk4_setup restated; the GPU tests hold it to results().max_syncs) and its
    carried-sync list"""
    row = ROWS[proto]
    ms = n // (row["sps"] - 1) + 2
    my = ms // row["win"] + 2
    myd = min(ms // 64 + 24 + 16, my + 16) if row["handlers"] else my + 16
    if row["gap"]:
        myd = min(myd, ms // row["gap"] + 4)
    return myd, 16


def cases():
    """(protocol, size) of the plain short-call cases"""
    return [(p, s) for p in ROWS for s in SIZES if s != "tiny" or p in TINY]


VOICE = ("dmr", "nxdn48", "ysf", "dpmr")
HANDLER_SIZES = ("below", "at")          # the DMR data-burst / embedded link control stream
MIXED_N, MIXED_CALLS = 8192, 7           # the mixed chain's DMR and NXDN48 groups: this many calls of one demodulator block

_STREAMS = {}


def _golden_iq(name):
    from conftest import golden
    return np.ascontiguousarray(golden(name)["iq"], np.uint8)


def _delay(iq, d, seed):
    rng = np.random.default_rng(seed)
    out = np.empty_like(iq)
    out[:d] = np.clip(np.rint(127.5 + rng.normal(0, 3, (d, 2))), 0, 255).astype(np.uint8)
    out[d:] = iq[:len(iq) - d]
    return out


def _batch(iq, L, delay, lo=0, later=None):
    """the stretch [lo, lo + L) of a capture: as sent, delayed, and negated (I/Q swapped: the other polarity) - or, where the protocol's
    configuration hunts one polarity only, the stretch that starts `later` samples further on"""
    a = iq[lo:lo + L]
    return np.stack([a, _delay(a, delay, 7), a[:, ::-1] if later is None else iq[lo + later:lo + later + L]])


def _dstar_generated(n_units, seed, neg):
    """a header unit and voice units back to back as 2-level FM cu8 (tests/dstar.py's encoders)"""
    import edacsgen
    rng = np.random.default_rng(seed)
    word = lambda wd: np.array([1.0 if ch == "1" else -1.0 for ch in wd], np.float32)
    parts = [np.tile(np.array([1.0, -1.0], np.float32), 40)]
    for k in range(n_units):
        if k == 0:
            h = dstar.make_header(0, "RPT2", "RPT1", "CQCQCQ", "N0CALL")
            parts += [word(dstar.WORDS[dstar.PAT_HD_NEG if neg else dstar.PAT_HD_POS]), dstar.header_air_symbols(h, neg, 1.0)]
        else:
            parts.append(word(dstar.WORDS[dstar.PAT_VOICE_NEG if neg else dstar.PAT_VOICE_POS]))
        fr = rng.integers(0, 2, (dstar.FRAMES, 4, 24)).astype(np.uint8)
        parts.append(dstar.bits_to_symbols(dstar.encode_voice(fr, dstar.encode_slow_data(bytes(rng.integers(0x20, 0x7F, 60).astype(np.uint8)))), neg, 1.0))
    parts.append(np.tile(np.array([1.0, -1.0], np.float32), 60))
    signs = np.sign(np.concatenate(parts)).astype(np.int8)
    return edacsgen.modulate_cu8(signs, len(signs) * 10 + 700, sps=10, dev=0.12, lead=300 + 77 * neg, seed=seed)


def stream(proto, kind="plain"):
    """the cu8 batch [B][samples][2] of a case: kind "plain" (below / at / block), "tiny" (a stretch of about six units), "voice"
    (vocoder = 1, one generated voice stream per protocol), "handlers" (DMR: data bursts of every kind and embedded link control),
    "mixed" (DMR, NXDN48: the start of the plain batch, as long as the mixed-chain case runs)"""
    key = (proto, kind)
    if key not in _STREAMS:
        _STREAMS[key] = _build(proto, kind)
    return _STREAMS[key]


def _build(proto, kind):
    import p25gen
    rng = np.random.default_rng(1000 + sorted(ROWS).index(proto))
    tiny = kind == "tiny"
    if kind == "mixed":
        return np.ascontiguousarray(stream(proto, "plain")[:, :MIXED_N * MIXED_CALLS])
    if kind == "handlers":
        dib, _ = dmr_data_stream(rng)
        vdib, _ = dmr_voice_stream(rng, 3)
        L = 10 * max(len(dib), len(vdib)) + 3000
        return np.stack([p25gen.modulate_cu8(dib, L, lead=300, seed=4, noise=0.02), p25gen.modulate_cu8(vdib, L, lead=433, seed=5, noise=0.02),
                         _delay(p25gen.modulate_cu8(dib, L, lead=300, seed=6, noise=0.02), 1234, 3)])
    if kind == "voice":
        if proto == "dmr":
            vdib, _ = dmr_voice_stream(rng, 3)
            L = 10 * len(vdib) + 3000
            return np.stack([p25gen.modulate_cu8(vdib, L, lead=300 + 211 * c, seed=5 + c, noise=0.02) for c in range(3)])
        if proto == "nxdn48":
            iq = _golden_iq("iq_nxdn48.npz")
            return np.stack([iq[60000 + 371 * c:60000 + 371 * c + 110000] for c in range(3)])
        if proto == "ysf":
            import ysfgen
            plan = [(0, 1, {}), (1, 0, dict(fn=1, ft=6)), (1, 2, dict(fn=2, ft=6)), (1, 0, dict(fn=3, ft=6)), (1, 2, dict(fn=4, ft=6, break_fich=True)),
                    (1, 3, dict(fn=0, ft=1)), (1, 3, dict(fn=1, ft=1)), (1, 3, dict(fn=2, ft=1)), (1, 2, dict(fn=5, ft=6)), (1, 0, dict(fn=6, ft=6)),
                    (1, 3, dict(fn=1, ft=6)), (1, 3, dict(fn=2, ft=6)), (1, 3, dict(fn=3, ft=6)), (1, 0, dict(fn=4, ft=6)), (1, 2, dict(fn=5, ft=6)),
                    (2, 1, {})]
            dib = np.concatenate([ysfgen.frame(rng, fi, dt, **kw) for fi, dt, kw in plan] + [rng.integers(0, 4, 80).astype(np.uint8)])
            return np.stack([p25gen.modulate_cu8(dib, 10 * len(dib) + 3000, lead=230 + 170 * c, seed=5 + c) for c in range(3)])
        if proto == "dpmr":
            import dpmrgen
            sfs = dpmr_voice_transmission(rng, DPMR_VOICE_PLAN[:8])
            out = []
            for c in range(3):
                dib = dpmrgen.transmission(sfs)
                out.append(p25gen.modulate_cu8(dib, 20 * len(dib) + 6000, sps=20, dev=0.045, lead=1000 + 333 * c, seed=c))
            return np.stack(out)
    if proto == "dmr":
        return _batch(_golden_iq("iq_dmr_t3_ras_cc.npz"), 14000 if tiny else 60000, 1234, later=20011)
    if proto == "nxdn48":
        return _batch(_golden_iq("iq_nxdn48.npz"), 36000 if tiny else 120000, 2345, lo=60000)
    if proto == "nxdn96":
        return _batch(_golden_iq("iq_nxdn96.npz"), 60000, 1234)
    if proto == "m17":
        # (a voice stream: LSF, then stream frames.  The delayed copy starts 137 samples earlier in the capture: noise in front of this
        # stretch costs the loop the preamble its polarity comes from)
        iq, L = _golden_iq("iq_m17.npz"), 24000 if tiny else 60000
        return np.stack([iq[78000:78000 + L], iq[78000 - 137:78000 - 137 + L], iq[78000:78000 + L, ::-1]])
    if proto == "ysf":
        return _batch(_golden_iq("iq_ysf.npz"), 80000, 1234)
    if proto == "dpmr":
        iq = _golden_iq("iq_dpmr.npz")[:, ::-1]          # (the capture is sent inverted: negated, -fm locks on every superframe)
        return _batch(iq, 120000, 2345, later=150007)
    if proto == "dstar":
        a, b = _dstar_generated(7, 3, 0), _dstar_generated(7, 4, 1)
        L = min(len(a), len(b))
        return np.stack([a[:L], b[:L], _delay(a[:L], 4321, 5)])
    if proto == "edacs":
        iq = _golden_iq("iq_edacs.npz")
        return _batch(iq, 11000 if tiny else 40000, 777)
    raise KeyError(key)


def loop_of(proto):
    """(front-end filter profile, a fresh oracle receive loop) as the chain configures the protocol"""
    if proto == "dmr":
        return 2, rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_DMR, rf_mod=2, handler=1))
    if proto in NXDN:
        return NXDN[proto]["lpf"], rx4.OracleFsk4Rx(rx4.profile(NXDN[proto]["proto"], rf_mod=NXDN[proto]["rf_mod"], handler=1))
    if proto == "m17":
        return 2, rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_M17))
    if proto == "ysf":
        return 2, rx4.OracleFsk4Rx(rx4.profile(rx4.PROTO_YSF))
    if proto == "dpmr":
        return 1, rx4.OracleFsk4Rx(dpmr.profile(0, rf_mod=2))
    if proto == "dstar":
        return 1, rx4.OracleFsk4Rx(dstar.profile(2))
    return 3, edacs.LoopRx(2)


def held_after_calls(proto, xc, n):
    """the records the loop holds after each call of n samples (the chain's d_new, summed): the oracle loop run call by call"""
    lpf, loop = loop_of(proto)
    disc = front_end_disc(xc, n, lpf)
    held, k = [], 0
    for a in range(0, len(disc), n):
        k += len(loop.run(disc[a:a + n], max_sync=n // 8 + 8)["sym"])
        held.append(k)
    return np.array(held, np.int64)


def stream_of(proto, size):
    return stream(proto, "tiny" if size == "tiny" else "plain")


# ---- one reference per (protocol, kind, size), shared by the tests that need it ------------------------------------------------------
_ORACLE = {}


def oracle_of(proto, kind, n):
    """per channel the whole-stream reference of stream(proto, kind) at calls of n samples"""
    key = (proto, kind, n)
    if key not in _ORACLE:
        x = stream(proto, kind)
        fn = {"dmr": dmr_oracle_stream, "nxdn48": lambda xc, m: nxdn_oracle_stream(xc, m, "nxdn48"),
              "nxdn96": lambda xc, m: nxdn_oracle_stream(xc, m, "nxdn96"), "m17": m17_oracle_stream, "ysf": ysf_oracle_stream,
              "dpmr": dpmr_oracle_stream, "dstar": dstar_oracle_stream, "edacs": edacs_loop_stream}[proto]
        _ORACLE[key] = [fn(x[c], n) for c in range(x.shape[0])]
    return _ORACLE[key]


def sync_positions(proto, want):
    """(all accepted syncs, the positions of the valid units) of one channel's reference"""
    if proto == "dmr":
        return [int(p) for p in want["w"]["sync_pos"]], [p for p, _ in dmr_units(want)]
    if proto in NXDN:
        return [int(p) for p in want["w"]["sync_pos"]], [f[0] for f in want["frames"]]
    if proto == "m17":
        return [f["pos"] for f in want[1]], [f["pos"] for f in want[1] if f["kind"] in ("lsf", "str")]
    if proto == "ysf":
        return [int(p) for p in want[0]["sync_pos"]], [f["pos"] for f in want[2] if f["payload"] is not None]
    if proto == "dpmr":
        return [int(p) for p in want[1]], [int(want[1][k]) for k, _ in want[2]]
    if proto == "dstar":
        return [int(p) for p in want[0]["sync_pos"]], [int(want[0]["sync_pos"][k]) for k, _ in want[1]]
    if proto == "edacs":
        return [int(p) for p in want["sync_pos"]], [int(p) for p in want["sync_pos"] if int(p) + 1 + edacs.FRAME <= len(want["sym"])]
    raise KeyError(proto)


def run_and_check(proto, kind, n, vocoder=0):
    """the chain over stream(proto, kind) in calls of n samples against oracle_of(): every channel, the drop counter included"""
    x = stream(proto, kind)
    want = oracle_of(proto, kind, n)
    info = {}
    B = x.shape[0]
    if proto == "dmr":
        run = dmr_run_chain(x, n, vocoder=vocoder, info=info)
        for c in range(B):
            dmr_check_chain_channel(run, c, want[c], vocoder)
    elif proto in NXDN:
        run = nxdn_run_chain(x, n, proto, vocoder=vocoder, info=info)
        for c in range(B):
            nxdn_check_chain_channel(run, c, want[c], vocoder)
    elif proto == "m17":
        run = m17_run_chain(x, n, info=info)
        for c in range(B):
            m17_check_chain_channel(run[c], want[c])
    elif proto == "ysf":
        run = ysf_run_chain(x, n, vocoder=vocoder, info=info)
        for c in range(B):
            ysf_check_chain_channel(run, c, want[c], vocoder)
    elif proto == "dpmr":
        sfs, voice, _ = dpmr_run_chain(x, n, vocoder=vocoder, info=info)
        for c in range(B):
            dpmr_check_chain_channel(sfs[c], want[c])
            if vocoder:
                dpmr_check_chain_voice(voice[c], want[c], c)
    elif proto == "dstar":
        run = dstar_run_chain(x, n, info=info)
        for c in range(B):
            dstar_check_chain_channel(run[c], want[c])
    else:
        run = edacs_run_chain(x, n, info=info)
        for c in range(B):
            edacs_check_chain_channel(run[c], want[c])
    check_info(info)
    return info
