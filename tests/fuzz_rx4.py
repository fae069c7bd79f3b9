"""Traffic builder of the fsk4 receive loop's protocol fuzz (tests/test_fuzz_rx4_protocols_gpu.py, tests/test_fuzz_rx4_traffic.py):
one table row per protocol (capture, oracle, draws of its own) and a builder that turns a (protocol, case) pair into a batch, its
per-channel lock lengths, its kernel shape, its sample rate and its call cuts.  TEST INFRASTRUCTURE - the product never imports this.

Slices at random offsets of the dPMR and D-STAR captures almost never hold a sync (6 syncs in 480 000 / 192 000 samples), so the
builder first runs the oracle over the whole capture (cached per capture) and starts every slice 300..3000 samples before a sync it
found.  At a sample rate other than the capture's the slices are only noise to the loop; the traffic that locks there is made of
symbols - the capture's own, as the oracle decided them, and the test generators' (edacsgen, dpmrgen, dstar.encode_*, ysfgen) - each
repeated samples-per-symbol times.  The same floats go to the device and to the oracle: nothing is resampled."""
import dataclasses
import os

import numpy as np

import dpmr
import dpmrgen
import dstar
import edacs
import edacsgen
import rx4
import ysfgen

BASE = int(os.environ.get("DDN_FUZZ_BASE", "0"))
N_CASES = 8
CPW = (1, 2, 4, 8, 16, 32)


@dataclasses.dataclass(frozen=True)
class Row:
    name: str
    gpu_proto: int          # ddn.FSK4_* (dsd-neo_amd/bindings/ddn.py)
    cap: str                # the capture under tests/golden and its front-end filter profile
    lpf: int
    sym_rate: int
    win_len: int            # symbols of the sync word
    frames: tuple           # in-frame symbols per lock class (the classes the protocol uses)
    rf_mod0: int            # the modulation rules the capture is scanned with
    salt: int               # the protocol's seed constant
    both: bool              # hunts both polarities
    sps_range: tuple        # samples per symbol ddn_fsk4_rx_create accepts
    sps_off: tuple          # the samples per symbol of the cases that leave 48 ksps
    draws: tuple = ()       # draws of its own

    def oracle(self, rf_mod, out_rate, lock, use_filter=1, inverted=0):
        """one channel's CPU loop; lock = the four per-class lengths"""
        lock = [int(v) for v in lock]
        if self.name == "edacs":
            return edacs.LoopRx(rf_mod=rf_mod, out_rate=out_rate, lock=lock[0])
        if self.name == "dpmr":
            return rx4.OracleFsk4Rx(dpmr.profile(inverted=inverted, use_filter=use_filter, rf_mod=rf_mod, lock=lock, out_rate=out_rate))
        if self.name == "dstar":
            return rx4.OracleFsk4Rx(dstar.profile(rf_mod, lock=lock, out_rate=out_rate))
        proto = {"nxdn96": rx4.PROTO_NXDN96, "m17": rx4.PROTO_M17, "ysf": rx4.PROTO_YSF}[self.name]
        return rx4.OracleFsk4Rx(rx4.profile(proto, rf_mod=rf_mod, use_filter=use_filter, lock=lock, out_rate=out_rate))

    def default_lock(self):
        return list(self.frames) + [0] * (4 - len(self.frames))


_C4FM = dict(sym_rate=4800, sps_range=(8, 21), sps_off=(8, 9, 11, 16, 21))
ROWS = {r.name: r for r in (
    Row(name="nxdn96", gpu_proto=3, cap="iq_nxdn96.npz", lpf=2, win_len=10, frames=(182,), rf_mod0=0, salt=1100, both=True,
        draws=("use_filter",), **_C4FM),
    Row(name="m17", gpu_proto=4, cap="iq_m17.npz", lpf=2, win_len=8, frames=(184, 8), rf_mod0=0, salt=1200, both=True, **_C4FM),
    Row(name="ysf", gpu_proto=5, cap="iq_ysf.npz", lpf=2, win_len=20, frames=(460,), rf_mod0=0, salt=1300, both=True,
        draws=("use_filter",), **_C4FM),
    Row(name="dpmr", gpu_proto=6, cap="iq_dpmr.npz", lpf=1, win_len=12, frames=(372,), rf_mod0=2, salt=1400, both=False,
        draws=("inverted", "use_filter"), sym_rate=2400, sps_range=(8, 21), sps_off=(8, 9, 11, 16, 21)),
    Row(name="dstar", gpu_proto=7, cap="iq_dstar.npz", lpf=1, win_len=24, frames=(dstar.HEADER_SYMS + dstar.VOICE_SYMS, dstar.VOICE_SYMS),
        rf_mod0=2, salt=1500, both=True, **_C4FM),
    Row(name="edacs", gpu_proto=8, cap="iq_edacs.npz", lpf=3, win_len=48, frames=(edacs.FRAME,), rf_mod0=2, salt=1600, both=True,
        sym_rate=9600, sps_range=(5, 10), sps_off=(6, 7, 8, 10)),
)}
PROTOCOLS = tuple(ROWS)


def max_symbols(n, sps):
    """ddn_fsk4_rx_max_symbols restated (the GPU test checks it against the library)"""
    return n // (sps - 1) + 2


def max_syncs(n, sps, win_len):
    return max_symbols(n, sps) // win_len + 2


# ---- the oracle over the whole capture, once per capture ------------------------------------------------------------------------------
_SCAN = {}


def run_chunked(orc_rx, x, step):
    """the oracle over x in calls of `step` samples -> (concatenated output, symbols held after each call)"""
    parts, held, k = [], [], 0
    for a in range(0, len(x), step):
        o = orc_rx.run(x[a:a + step], max_sync=step // 8 + 4)
        o["sync_pos"] = o["sync_pos"] + k
        k += len(o["sym"])
        parts.append(o)
        held.append(k)
    out = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    return out, np.array(held)


def scan(name):
    """-> dict(disc, sym, fl, sync_pos, sync_pat, sync_at = the sample (to 500) at which each sync was accepted, level, rows = the
    (pattern row, sign) pairs the capture yields as it is (sign 1) and negated (sign -1))"""
    if name not in _SCAN:
        row = ROWS[name]
        disc = rx4.capture_disc(row.cap, row.lpf)
        out, held = run_chunked(row.oracle(row.rf_mod0, 48000, row.default_lock()), disc, 500)
        at = np.searchsorted(held, out["sync_pos"], side="right") * 500
        inframe = out["sym"][(out["fl"] & 1) == 1]
        level = float(np.percentile(np.abs(inframe), 90)) if len(inframe) else 1.0
        rows = [(int(p), 1) for p in sorted(set(out["sync_pat"].tolist()))]
        neg = None
        if row.both:
            neg, _ = run_chunked(row.oracle(row.rf_mod0, 48000, row.default_lock()), -disc, 1 << 20)
            rows += [(int(p), -1) for p in sorted(set(neg["sync_pat"].tolist()))]
        _SCAN[name] = dict(disc=disc, sym=out["sym"], fl=out["fl"], sync_pos=out["sync_pos"], sync_pat=out["sync_pat"], sync_at=at,
                           level=level, rows=rows, neg=neg)
    return _SCAN[name]


# ---- symbol streams (one float per symbol), repeated samples-per-symbol times by the builder --------------------------------------------
_LEVEL4 = np.array([1.0, 3.0, -1.0, -3.0], np.float32) / 3.0        # dibit -> symbol level (0 = +1, 1 = +3, 2 = -1, 3 = -3)


def capture_symbols(name, rng, target=None):
    """a run of the capture's own symbols round one to three of its syncs, two syncs of context first where the capture has them;
    target = (pattern row, sign): a sync of that row is among them"""
    s = scan(name)
    row = ROWS[name]
    pos, pat, sym = s["sync_pos"], s["sync_pat"], s["sym"]
    if target is not None:
        if target[1] < 0:
            pos, pat, sym = s["neg"]["sync_pos"], s["neg"]["sync_pat"], s["neg"]["sym"]
        hits = np.flatnonzero(pat == target[0])
        i = int(hits[int(rng.integers(0, len(hits)))])
    else:
        i = int(rng.integers(0, len(pos)))
    first = max(0, i - 2)
    last = min(len(pos) - 1, i + int(rng.integers(0, 2)))
    a = max(0, max(int(pos[first]), int(pos[i]) - 450) - row.win_len - int(rng.integers(30, 120)))
    b = min(len(sym), int(pos[last]) + 1 + int(rng.integers(20, min(2 * row.frames[0], 400) + 40)))
    return sym[a:b]


def dense_symbols(name, rng, n_sym, lock):
    """sync words as close together as the lock lengths `lock` let them all count - each with that many symbols of the capture behind
    it, now and then up to 60 more: many hunt <-> frame transitions in few samples"""
    s = scan(name)
    row = ROWS[name]
    cls = lambda pat: (0 if pat >= 2 else 1) if len(row.frames) == 2 else 0       # (M17, D-STAR: rows 0 / 1 are the second class)
    out, k = [s["sym"][max(0, int(s["sync_pos"][0]) - row.win_len - 60):int(s["sync_pos"][0]) - row.win_len + 1]], 0
    while k < n_sym:
        i = int(rng.integers(0, len(s["sync_pos"])))
        a = int(s["sync_pos"][i]) - row.win_len + 1
        seg = s["sym"][max(0, a - int(rng.integers(0, 6))):a + row.win_len + int(lock[cls(int(s["sync_pat"][i]))])
                       + int(rng.integers(0, 8) if rng.random() < 0.8 else rng.integers(8, 60))]
        out.append(seg)
        k += len(seg)
    return np.concatenate(out)[:max(n_sym, 1)]


def generated_symbols(name, rng, level, inverted=0):
    """a transmission from the protocol's test generator as symbol levels, or None where the protocol has none"""
    lv = np.float32(level)
    lead = np.tile(np.array([1.0, -1.0], np.float32), 24) * lv
    if name == "edacs":
        signs, _ = edacsgen.stream(rng, int(rng.integers(2, 6)), int(rng.integers(0, 2)), gap=(0, 24))
        return np.concatenate([lead, signs.astype(np.float32) * lv])
    if name == "dpmr":
        sf = [rng.integers(0, 4, dpmr.FRAME).astype(np.uint8) for _ in range(int(rng.integers(2, 4)))]
        return np.concatenate([lead, _LEVEL4[dpmrgen.transmission(sf, inverted=bool(inverted))] * lv])
    if name == "ysf":
        d = np.concatenate([ysfgen.frame(rng, int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(int(rng.integers(2, 4)))])
        return np.concatenate([lead, _LEVEL4[d] * lv * np.float32(rng.choice([1.0, -1.0]))])
    if name == "dstar":
        neg = int(rng.integers(0, 2))
        word = lambda w: np.array([1.0 if ch == "1" else -1.0 for ch in w], np.float32) * lv
        parts = [lead]
        if rng.integers(0, 2):
            h = dstar.make_header(0, "RPT2", "RPT1", "CQCQCQ", "N0CALL", good_crc=bool(rng.integers(0, 2)))
            parts += [word(dstar.WORDS[dstar.PAT_HD_NEG if neg else dstar.PAT_HD_POS]), dstar.header_air_symbols(h, neg, float(lv))]
        else:
            parts.append(word(dstar.WORDS[dstar.PAT_VOICE_NEG if neg else dstar.PAT_VOICE_POS]))
        fr = rng.integers(0, 2, (dstar.FRAMES, 4, 24)).astype(np.uint8)
        v = dstar.encode_voice(fr, dstar.encode_slow_data(bytes(rng.integers(0, 256, 60).astype(np.uint8))))
        parts.append(dstar.bits_to_symbols(v, neg, float(lv)))
        parts.append(word(dstar.WORDS[dstar.PAT_VOICE_NEG if neg else dstar.PAT_VOICE_POS]))
        parts.append(dstar.bits_to_symbols(rng.integers(0, 2, int(rng.integers(100, 400))), neg, float(lv)))
        return np.concatenate(parts).astype(np.float32)
    return None


# ---- one case -------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def lock_options(frame):
    """{0, a tenth of the frame, the frame, twice the frame}"""
    return [0, max(1, frame // 10), frame, 2 * frame]


def _off_rate_sps(row, base):
    """the samples per symbol of a protocol's four cases off 48 ksps: the ends of the accepted range that 48 ksps is not, the rest drawn"""
    r = np.random.default_rng(7000 * base + row.salt)
    ends = [v for v in row.sps_range if v in row.sps_off]
    rest = [v for v in row.sps_off if v not in ends]
    v = ends + [int(x) for x in r.choice(rest, 4 - len(ends))]
    return [v[i] for i in r.permutation(4)]


def tile_of(cpw):
    """the staging tile of the kernel's Lds4: 128 samples up to 8 channels per wavefront, 64 from 16 on; its ring is indexed from the
    start of each call, so a call meets a tile edge through its LENGTH"""
    return 128 if cpw <= 8 else 64


def _cpw_of(row, case, base):
    """channels per wavefront from a stream of its own; every shape once in a protocol's eight cases, two drawn freely"""
    r = np.random.default_rng(5000 * base + row.salt)
    v = [CPW[i] for i in r.permutation(6)] + [int(x) for x in r.choice(CPW, 2)]
    return v[case]


def sync_end_samples(orc_rx, x, limit=4):
    """the sample that ends the last symbol of a sync word, for up to `limit` syncs of x: the oracle in calls of 256 samples, the call
    that holds a sync taken again sample by sample from a copy of the state before it"""
    import ctypes as C
    ends = []
    for a in range(0, len(x), 256):
        before = bytes(orc_rx.st.raw)
        o = orc_rx.run(x[a:a + 256], max_sync=40)
        if len(o["sync_pos"]) and len(ends) < limit:
            after = bytes(orc_rx.st.raw)
            C.memmove(orc_rx.st, before, len(before))
            for k in range(a, min(a + 256, len(x))):
                if len(orc_rx.run(x[k:k + 1], max_sync=4)["sync_pos"]):
                    ends.append(k)
            C.memmove(orc_rx.st, after, len(after))
    return ends


def _channel(c, rng, ch):
    """one channel's samples: segments of capture slices and symbol streams (scaled, noisy), pure noise, silence and gaps long enough
    for the carrier-loss timeout; channel 0 opens with sync words close together behind the case's target rows"""
    row, n, sps, name = c.row, c.n, c.sps, c.name
    s = scan(name)
    targets = s["rows"]
    native = c.out_rate == 48000
    pol = np.float32(-1.0 if c.inverted else 1.0)       # (-xd hunts the inverted word: the capture is sent negated)
    x = np.zeros(n, np.float32)
    pos, seg_no = 0, 0
    while pos < n:
        kind = rng.random()
        ln = min(int(rng.integers(500, 30000)), n - pos)
        scale = np.float32(rng.choice([1.0, -1.0, 0.4, 1.7]))
        noise = np.float32(rng.choice([0, 150, 900]))
        if seg_no == 0 and ch == 0:
            ln = min(n - pos, max(ln, n // 2))
            head, room = [], ln // sps // 2             # (at least half of the segment stays for the close sync words)
            for j in range(3):
                h = capture_symbols(name, rng, targets[(c.case + N_CASES * j) % len(targets)]) * pol
                if len(h) > room:
                    break
                room -= len(h)
                head += [h, np.zeros(int(rng.integers(4, 40)), np.float32)]
                if len(targets) <= N_CASES * (j + 1):
                    break
            sy = np.concatenate(head + [dense_symbols(name, rng, ln // sps + 1, c.lock[0]) * pol])
            seg = np.repeat(sy, sps)[:ln]
            ln = len(seg)
            seg = seg + rng.standard_normal(ln).astype(np.float32) * noise
        elif kind < 0.6:
            how = rng.random()
            if native and how < 0.5:
                at = int(s["sync_at"][int(rng.integers(0, len(s["sync_at"])))]) - int(rng.integers(300, 3000))
                at = max(0, min(at, len(s["disc"]) - ln))
                seg = s["disc"][at:at + ln] * scale * pol
            elif not native and how < 0.2:
                at = int(rng.integers(0, len(s["disc"]) - ln))
                seg = s["disc"][at:at + ln] * scale * pol
            else:
                t = targets[int(rng.integers(0, len(targets)))]
                gen = generated_symbols(name, rng, s["level"], c.inverted) if how > 0.8 else None
                if gen is None:
                    gen = capture_symbols(name, rng, t) * pol
                    scale = abs(scale)                  # (the target row names the polarity)
                seg = np.repeat(gen, sps)[:ln] * scale
                ln = len(seg)
            seg = seg + rng.standard_normal(ln).astype(np.float32) * noise
        elif kind < 0.75:
            seg = rng.standard_normal(ln).astype(np.float32) * np.float32(rng.choice([50, 2000, 12000]))
        elif kind < 0.87:
            seg = np.zeros(ln, np.float32)
        else:
            # a gap long enough for the carrier-loss timeout (1800 hunting symbols), where it still fits
            ln = min(1800 * sps + int(rng.integers(100, 2000)), n - pos)
            seg = np.zeros(ln, np.float32) if rng.integers(0, 2) else rng.standard_normal(ln).astype(np.float32) * np.float32(300)
        x[pos:pos + ln] = seg
        pos += ln
        seg_no += 1
    return x


def _cuts(c, rng):
    """call cuts: 0..3 random ones, a call of one sample, a call shorter than a symbol, a cut one sample behind the sample that ends a
    sync's last symbol (channel 0, positions from the oracle) and - last, so that no other cut falls into them - two calls whose LENGTH
    is a multiple of the case's staging tile -1, +0 or +1; the call behind each starts on that edge of the stream's own"""
    n, sps = c.n, c.sps
    cuts = {0: "", n: ""}
    for v in rng.integers(1, n, int(rng.integers(0, 4))):
        cuts.setdefault(int(v), "random")
    a = int(rng.integers(1, n - 2))
    cuts[a], cuts[a + 1] = cuts.get(a, "one-sample"), "one-sample"
    a = int(rng.integers(1, n - sps))
    cuts[a], cuts[a + int(rng.integers(2, sps - 1))] = cuts.get(a, "sub-symbol"), "sub-symbol"
    c.sync_ends = sync_end_samples(c.row.oracle(c.rf_mod, c.out_rate, c.lock[0], c.use_filter, c.inverted), c.x[0])
    if c.sync_ends:
        e = c.sync_ends[int(rng.integers(0, len(c.sync_ends)))]
        if e + 2 < n:
            cuts.setdefault(e + 1, "sync-end")          # the call ends with the sync's last symbol, and one sample after it
            cuts[e + 2] = "sync-end"
    tile = tile_of(c.cpw)
    c.tile_calls = []
    for d in rng.permutation([-1, 0, 1])[:2]:
        at = sorted(cuts)
        room = [(p, q) for p, q in zip(at[:-1], at[1:]) if q - p > tile + 2 and (p, q) not in c.tile_calls]
        if not room:
            break
        p, q = room[int(rng.integers(0, len(room)))]
        cut = p + tile * int(rng.integers(1, (q - p - 2) // tile + 1)) + int(d)
        cuts[cut] = "tile"
        c.tile_calls.append((p, cut))
    c.kinds = cuts
    c.cuts = sorted(cuts)


def build(name, case, base=BASE):
    """-> Case: row, seed, B, n, rf_mod, use_filter, inverted, cpw, sps, out_rate, lock [B][4], x [B][n], cuts, kinds (what each cut
    is there for), tile_calls, sync_ends, lock_choice [B][classes] (index into lock_options)"""
    row = ROWS[name]
    c = Case()
    c.row, c.name, c.case = row, name, case
    c.seed = 1000 * base + case + row.salt
    rng = np.random.default_rng(c.seed)
    c.B = B = int(rng.choice([1, 3, 9, 17, 40]))
    c.n = int(rng.integers(9000, 60000))
    c.rf_mod = int(rng.choice([0, 2]))
    c.use_filter = int(rng.integers(0, 2)) if "use_filter" in row.draws else 1
    c.inverted = int(rng.integers(0, 2)) if "inverted" in row.draws else 0
    c.cpw = _cpw_of(row, case, base)
    if c.cpw >= 8 and B < 3:
        # a wide wavefront shape with one channel has one live lane: a lane-indexing error of that shape would not show
        c.B = B = int(np.random.default_rng(6000 * base + case + row.salt).choice([3, 9, 17, 40]))
    c.sps = 48000 // row.sym_rate if case % 2 == 0 else _off_rate_sps(row, base)[case // 2]
    c.out_rate = row.sym_rate * c.sps
    # lock lengths: channel 0, which carries the close sync words, keeps a tenth of the frame; everything else draws all four options
    nclass = len(row.frames)
    c.lock_choice = np.zeros((B, nclass), np.int32)
    c.lock = np.zeros((B, 4), np.int32)
    for ch in range(B):
        for k in range(nclass):
            j = int(rng.integers(0, 4))
            if ch == 0:                                 # (short, so the close sync words all count; never all 0: in-frame symbols)
                j = 1 if k == nclass - 1 else j & 1
            c.lock_choice[ch, k] = j
            c.lock[ch, k] = lock_options(row.frames[k])[j]
        if not c.lock[ch].any():
            c.lock[ch, 3] = 7                           # lock 0 with another entry non-zero (an unused class)
    c.x = np.stack([_channel(c, rng, ch) for ch in range(B)])
    _cuts(c, rng)
    return c


def oracles(c):
    return [c.row.oracle(c.rf_mod, c.out_rate, c.lock[ch], c.use_filter, c.inverted) for ch in range(c.B)]


def calls(c):
    return list(zip(c.cuts[:-1], c.cuts[1:]))


def build_densest(name, base=BASE):
    """-> Case: the streams that fill the sync table furthest - lock lengths of one symbol, the fewest samples per symbol the loop
    accepts, every channel sync words one lock symbol apart; channel 0 of M17 a long preamble, of EDACS frames back to back"""
    row = ROWS[name]
    c = Case()
    c.row, c.name, c.case = row, name, "densest"
    c.seed = 1000 * base + row.salt + 99
    rng = np.random.default_rng(c.seed)
    c.B, c.rf_mod, c.use_filter, c.inverted, c.cpw = 9, row.rf_mod0, 1, 0, 8
    c.sps = 5 if name == "edacs" else 8
    if name == "dpmr":
        c.use_filter = 0        # (dpmr_filter's taps are fixed ones for 20 samples per symbol: at 8 nothing locks behind it)
    c.out_rate = row.sym_rate * c.sps
    n_sym = 3000
    c.n = n_sym * c.sps
    c.lock = np.zeros((c.B, 4), np.int32)
    c.lock[:, :len(row.frames)] = 1
    s = scan(name)
    x = np.zeros((c.B, c.n), np.float32)
    for ch in range(c.B):
        sy = dense_symbols(name, rng, n_sym, c.lock[ch])
        if row.both and ch % 2:
            sy = -sy
        if ch == 0 and name == "m17":
            sy = np.tile(np.array([1.0, -1.0], np.float32), n_sym // 2) * np.float32(s["level"])
        if ch == 0 and name == "edacs":
            sy = edacsgen.stream(rng, n_sym // 288 + 1, edacs.PAT_POS, gap=(0, 0))[0][:n_sym].astype(np.float32) * np.float32(s["level"])
        x[ch] = np.repeat(sy, c.sps)[:c.n]
    c.x = x
    c.cuts = [0, c.n // 3 + 1, c.n]
    c.kinds, c.sync_ends, c.tile_calls = {}, [], []
    return c
