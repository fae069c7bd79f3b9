"""CPU restatement of the reference's dPMR voice superframe path (-fm) for the tests: the receive-loop profile, the CCH decode
(descramble, 6 x 12 de-interleave, Hamming(12,8), CRC7, fields), the air-interface ID string, the superframe-part rules and the
colour code.  TEST INFRASTRUCTURE - the product never imports this.

  FS2 word, profile      src/dsp/dsd_frame_sync.c:832-862, include/dsd-neo/core/sync_patterns.h:123-132, decode_mode.c:459-483
  superframe layout      src/protocol/dpmr/dpmr_voice.c:397-425 (CCH 36, 4 x 36 AMBE, colour code 12, CCH 36, 4 x 36 AMBE)
  CCH decode             dpmr_voice.c:139-178, scrambler dpmr_data.c:80-117, de-interleave :431-452, CRC7 :455-474
  identity               dpmr_voice.c:182-274, AI-ID string :477-546
  colour code            dpmr_data.c (table: tests/golden/dpmr_vectors.json)
Hamming(12,8) goes through the oracle's decoder, which tests/test_fec3*.py pin to the compiled fec.c."""
import json
import os
import re

import numpy as np

import fec3
import rx4

FS2 = "113333131331"
FS2_INV = "331111313113"
T_FS2_POS, T_FS2_NEG = 22, 26          # synctype_ids.h:92,96 + 1 (0 stays "none")
FRAME = 372                            # dibits processdPMRvoice() reads behind FS2
PERIOD = 384                           # FS2 + 372
CCH0, CC_AT, CCH1 = 0, 180, 192        # dibit offsets behind the sync
VOICE_AT = (36, 72, 108, 144, 228, 264, 300, 336)
HERE = os.path.dirname(os.path.abspath(__file__))


def vectors():
    return json.load(open(os.path.join(HERE, "golden", "dpmr_vectors.json")))


def dpmr_taps():
    """bit patterns of the generated table (dsd-neo_amd/csrc/ddn_tables_dpmr.h)"""
    txt = open(os.path.join(HERE, "..", "dsd-neo_amd", "csrc", "ddn_tables_dpmr.h")).read()
    m = re.search(r"ddn_dpmr_filter_bits\[[A-Z0-9_]+\] = \{(.*?)\};", txt, re.S)
    return [int(x.rstrip("u"), 16) for x in re.findall(r"0x[0-9a-f]+u", m.group(1))]


def profile(inverted=0, use_filter=1, rf_mod=2, lock=None, out_rate=48000):
    """the loop profile ddn_fsk4_rx_create builds for DDN_FSK4_DPMR (tests/rx4.py's Profile).

    rf_mod defaults to 2 (the GFSK window / slip / clip rules): under -fm without a modulation lock the reference's hunt profile
    2400_4 "uses GFSK exclusively" (frame_sync_profile_uses_gfsk_exclusively(), src/dsp/dsd_frame_sync.c:2338-2356), so
    frame_sync_active_profile_modulation() (:2359-2374) wants modulation 2 at every check, one vote switches (:1910-1927) and
    nothing votes back (the C4FM / QPSK candidates are off on 2400_4, :1842-1860).  The first check falls t_max = 12 hunting symbols
    into the stream (frame_sync_maybe_auto_switch_modulation(), :1952-1975); the loop holds the GFSK rules from symbol 0."""
    p = rx4.Profile()
    p.proto, p.handler = rx4.PROTO_P25P1, 0     # (no handler family: a fixed count)
    p.out_rate, p.rf_mod, p.use_filter = out_rate, rf_mod, use_filter
    p.sym_rate, p.win_len, p.t_max, p.warm_len = 2400, 12, 12, 12
    p.n_pat = 1
    p.pat_bits[0] = rx4.bits_of(FS2_INV if inverted else FS2)
    p.pat_type[0] = T_FS2_NEG if inverted else T_FS2_POS
    p.pat_neg[0], p.pat_class[0] = 0, 0         # not a four-level negative type to digitize(): dibits stay as sliced
    taps = dpmr_taps()
    p.nt = len(taps)
    for k, t in enumerate(taps):
        p.taps[k] = t
    for k, v in enumerate(lock or [FRAME, 0, 0, 0]):
        p.lock_symbols[k] = v
    return p


def scramble(bits, seed=0x1FF):
    """x^9 + x^5 + 1 -> (output bits, advanced state)"""
    sh = [(seed >> i) & 1 for i in range(9)]
    out = []
    for b in bits:
        out.append((int(b) ^ sh[0]) & 1)
        fb = sh[4] ^ sh[0]
        sh = sh[1:] + [fb]
    return out, sum(v << i for i, v in enumerate(sh))


def deinterleave(bits72):
    return [bits72[i * 6 + j] for j in range(6) for i in range(12)]


def crc7(bits):
    s = 0
    for b in bits:
        s = (((s << 1) ^ 0x09) & 0x7F) if (((s >> 6) & 1) ^ int(b)) else ((s << 1) & 0x7F)
    return s


def cch_crc(bits48):
    return value(bits48[41:48])


def value(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v


def air_interface_id(v):
    s = ""
    for d in (1464100, 146410, 14641, 1331, 121, 11, 1):
        q, v = v // d, v % d
        s += "*" if q == 10 else str(q)
    return s


def color_code(bits24, table=None):
    code = value(bits24) | 0x555555
    for c, col in (table or vectors()["color_codes"]):
        if c == code:
            return col
    return -1


def dibit_bits(dibits):
    out = []
    for d in dibits:
        out += [(int(d) >> 1) & 1, int(d) & 1]
    return out


def decode_cch(dibits36):
    """-> dict(bits48, ham [6], ham_ok, crc_ok, fn, mode, version, format, emergency, reserved, slow)"""
    di = deinterleave(scramble(dibit_bits(dibits36))[0])
    _, dec, ok = fec3.oracle_decode(1, np.array(di, np.uint8).reshape(6, 12))
    b = dec.reshape(-1)
    return dict(bits48=b, ham=ok.astype(int).tolist(), ham_ok=bool(ok.all()), crc_ok=crc7(b[:41]) == cch_crc(b), fn=value(b[0:2]),
                mode=value(b[14:17]), version=value(b[17:19]), format=value(b[19:21]), emergency=int(b[21]), reserved=int(b[22]),
                slow=value(b[23:41]))


def superframe(dibits372, inverted=0):
    """the fields processdPMRvoice() forms from the 372 dibits behind FS2 (dpmr_read_dibit: XOR 2 under -xd)"""
    d = [int(x) ^ (2 if inverted else 0) for x in dibits372]
    c0, c1 = decode_cch(d[CCH0:CCH0 + 36]), decode_cch(d[CCH1:CCH1 + 36])
    idv = ((value(c0["bits48"][2:14]) << 12) & 0xFFF000) | (value(c1["bits48"][2:14]) & 0xFFF)
    return dict(cch=(c0, c1), id=idv, color=color_code(dibit_bits(d[CC_AT:CC_AT + 12])), voice=[d[a:a + 36] for a in VOICE_AT])


def part_of(sf):
    """the dpmr_superframe_part dpmr_extract_superframe_part() forms (dpmr_voice.c:180-195)"""
    c0, c1 = sf["cch"]
    return dict(fn=[c0["fn"], c1["fn"]], id=sf["id"], crc_ok=[int(c0["crc_ok"]), int(c1["crc_ok"])],
                ham_ok=[[c0["ham"][0], c0["ham"][1]], [c1["ham"][0], c1["ham"][1]]])


def update_part(state, part):
    """dpmr_update_superframe_part() on the identity state {tg, src, next} -> the kind ("called" | "calling" | None); a strong ID
    is published (TG for the called ID, Src for the calling one), a weak one leaves the state's IDs alone"""
    crc, ham, fn = part["crc_ok"], part["ham_ok"], part["fn"]
    strong = (crc[0] or (ham[0][0] and ham[0][1])) and (crc[1] or (ham[1][0] and ham[1][1]))
    kind = None
    if ((crc[0] or ham[0][0]) and fn[0] == 0) or ((crc[1] or ham[1][0]) and fn[1] == 1):
        kind, state["next"] = "called", 2
    elif ((crc[0] or ham[0][0]) and fn[0] == 2) or ((crc[1] or ham[1][0]) and fn[1] == 3):
        kind, state["next"] = "calling", 1
    else:
        state["next"] = {1: 2, 2: 1}.get(state.get("next", 0), 0)
    if kind and strong:
        state["tg" if kind == "called" else "src"] = air_interface_id(part["id"])
    return kind, bool(strong)


def part_rule(sf):
    """-> (kind, strong) of one superframe"""
    return update_part({}, part_of(sf))


def voice_plan(modes, versions, key=0):
    """dpmr_play_voice_frames() (dpmr_voice.c:354-395): frames synthesised per half (4 where the communication mode is 0, 1 or 5)
    and whether the last synthesised half was muted (version 3 = scrambled, muted unless a key is set)"""
    frames, muted = [], None
    for o in range(2):
        on = modes[o] in (0, 1, 5)
        frames.append(4 if on else 0)
        if on:
            muted = 1 if (versions[o] == 3 and not key) else 0
    return frames, muted


def voice_halves(sf):
    """which halves of a superframe are synthesised"""
    return [f > 0 for f in voice_plan([c["mode"] for c in sf["cch"]], [c["version"] for c in sf["cch"]])[0]]


def decode_stream(rec_dibits, sync_pos, inverted=0):
    """every whole superframe behind the loop's syncs -> list of (sync index, superframe dict); the identity state the reference's
    call state carries (TG, Src) as it stands after each"""
    out, st = [], {"tg": None, "src": None, "next": 0}
    for k, q in enumerate(sync_pos):
        q = int(q)
        if q + 1 + FRAME > len(rec_dibits):
            continue
        sf = superframe(rec_dibits[q + 1:q + 1 + FRAME], inverted)
        kind, strong = update_part(st, part_of(sf))
        sf["tg"], sf["src"], sf["kind"], sf["strong"] = st["tg"], st["src"], kind, strong
        out.append((k, sf))
    return out
