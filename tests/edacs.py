"""CPU restatement of the EDACS control-channel frame decode (DDN_FSK4_EDACS, ddn_edacs.hip) from the reference's definitions:
edacs() / edacs_build_raw_frames() / edacs_vote_frames() / edacs_process_valid_frame() and the message-type and site-ID fields of
src/protocol/edacs/edacs-fme.c, the BCH(40,28) code of edacs_bch() (src/protocol/edacs/edacs-bch3.c, restated from the code's
generator polynomial, checked against the reference's own test vectors in tests/golden/edacs_vectors.json) and the two-level slice of
store_two_level_dibit() (src/core/frames/dsd_dibit.c:938-948).  TEST INFRASTRUCTURE."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FRAME = 240
PAT_NEG, PAT_POS = 0, 1        # loop pattern index: 0 = EDACS_SYNC (accepted as -EDACS), 1 = INV_EDACS_SYNC (+EDACS)
GEN = 0x1539                   # x^12 + x^10 + x^8 + x^5 + x^4 + x^3 + 1
MASK40 = (1 << 40) - 1
ESK = 0xA0
MODES = {"-fh": (0, 0), "-fH": (0, ESK), "-fe": (1, 0), "-fE": (1, ESK)}


def vectors():
    return json.load(open(os.path.join(HERE, "golden", "edacs_vectors.json")))


def sync_word(pat):
    """the 48-symbol word ('1' / '3') the loop hunts as pattern `pat`"""
    w = vectors()["sync_words"]
    return w["EDACS_SYNC" if pat == PAT_NEG else "INV_EDACS_SYNC"]["symbols"]


def bch(msg):
    """edacs_bch(): the systematic BCH(40,28) codeword, message bits 27..0 above the 12 parity bits (bits above 27 ignored)"""
    msg &= 0x0FFFFFFF
    r = msg << 12
    for b in range(39, 11, -1):
        if (r >> b) & 1:
            r ^= GEN << (b - 12)
    return (msg << 12) | (r & 0xFFF)


def vote(a, b, c):
    """edacs_vote_frames(): bitwise majority of three copies, the middle one sent inverted"""
    b = ~b & MASK40
    return ((a & b) | (a & c) | (b & c)) & MASK40


def slice_bits(syms, center, pat):
    """store_two_level_dibit(): after +EDACS (pattern 1) a symbol above the center is a 0, after -EDACS (pattern 0) a 1"""
    high = np.asarray(syms, np.float32) > np.float32(center)
    return (high if pat == PAT_NEG else ~high).astype(np.uint8)


def words_of(bits240):
    """edacs_build_raw_frames(): six 40-bit words, the first bit received the most significant"""
    out = []
    for j in range(6):
        v = 0
        for b in bits240[40 * j:40 * (j + 1)]:
            v = (v << 1) | int(b)
        out.append(v)
    return out


def classify(m1, ea_mode, frame_ok):
    """-> (kind, types3, site6) as ddn_edacs_frame_decode_batch writes them"""
    if ea_mode:
        t = [(m1 >> 23) & 0x1F, (m1 >> 19) & 0xF, 0]
        site = t[0] == 0x1F and t[1] == 0xA
        f = [((m1 & 0x7000) >> 7) | (m1 & 0x1F), (m1 & 0xFE0) >> 5, 0, 0, 0, 0]
    else:
        t = [(m1 >> 25) & 7, (m1 >> 22) & 7, (m1 >> 17) & 0x1F]
        site = t[0] == 7 and t[1] == 7 and 0x08 <= t[2] <= 0x0B
        f = [m1 & 0x1F, (m1 >> 9) & 7, (m1 >> 12) & 0x1F, (m1 >> 7) & 1, (m1 >> 6) & 1, (m1 >> 5) & 1]
    site = site and frame_ok
    kind = ((2 if ea_mode else 1) + (2 if site else 0)) if frame_ok else 0
    return kind, t, f if site else [0] * 6


def decode_bits(bits240, ea_mode=0, esk_mask=0):
    """edacs() on 240 bits -> dict of every field the device kernel writes"""
    w = words_of(bits240)
    v = [vote(w[0], w[1], w[2]), vote(w[3], w[4], w[5])]
    ok = [int(bch(x >> 12) == x) for x in v]
    m = [(x >> 12) ^ (esk_mask << 20) for x in v]
    kind, t, f = classify(m[0], ea_mode, bool(ok[0] and ok[1]))
    return dict(raw40=w, vote40=v, bch_ok=ok, frame_ok=int(ok[0] and ok[1]), msg28=m, kind=kind, types=t, site6=f, valid=1)


def decode_slot(syms, pos, pat, thr5, ea_mode=0, esk_mask=0):
    """one sync slot of the device kernel: `syms` = the row's record symbols, `pos` = the sync's last symbol"""
    if pat > 1 or pos < 0 or pos + 1 + FRAME > len(syms):
        return dict(raw40=[0] * 6, vote40=[0, 0], bch_ok=[0, 0], frame_ok=0, msg28=[0, 0], kind=0, types=[0, 0, 0], site6=[0] * 6, valid=0)
    return decode_bits(slice_bits(syms[pos + 1:pos + 1 + FRAME], thr5[0], pat), ea_mode, esk_mask)


def site_line(site_id):
    """what the reference prints for a standard site ID: "Site ID [%02X][%03d]" """
    return "Site ID [%02X][%03d]" % (site_id, site_id)


# ---- the 9600_2 hunt restated on the CPU (tests/edacs_rx.c, built against the oracle's exported helpers) ---------------------------
_LOOP = None


def _loop_lib():
    global _LOOP
    if _LOOP is None:
        import ctypes as C
        import hashlib
        import subprocess
        import tempfile
        import orc
        orc.oracle()                                    # (builds oracle/libddn_oracle.so where it is missing)
        src = os.path.join(HERE, "edacs_rx.c")
        odir = os.path.join(orc.ROOT, "oracle")
        tag = hashlib.sha1(open(src, "rb").read() + open(orc.ORACLE_SO, "rb").read()).hexdigest()[:12]
        so = os.path.join(tempfile.gettempdir(), "ddn_edacs_rx_%d_%s.so" % (os.getuid(), tag))
        if not os.path.exists(so):
            tmp = so + ".%d" % os.getpid()
            subprocess.check_call(["gcc", "-std=c11", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-mfma",
                                   "-mavx2", "-fno-math-errno", "-I", odir, src, orc.ORACLE_SO, "-Wl,-rpath," + odir, "-o", tmp])
            os.replace(tmp, so)
        lib = C.CDLL(so)
        lib.edrx_sizeof.restype = C.c_size_t
        lib.edrx_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p]
        lib.edrx_run.restype = C.c_long
        lib.edrx_run.argtypes = [C.c_void_p, C.c_void_p, C.c_long] + [C.c_void_p] * 4 + [C.c_long] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        lib.edrx_set_sync_thresholds.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.edrx_get_thresholds.argtypes = [C.c_void_p, C.c_void_p]
        _LOOP = lib
    return _LOOP


class LoopRx:
    """one channel of the restated EDACS receive loop; run() returns what rx4.OracleFsk4Rx.run() returns"""

    def __init__(self, rf_mod=2, out_rate=48000, lock=FRAME):
        import ctypes as C
        self.C, self.l = C, _loop_lib()
        self.st = C.create_string_buffer(self.l.edrx_sizeof())
        self.l.edrx_init(self.st, out_rate, rf_mod, lock, sync_word(PAT_NEG).encode(), sync_word(PAT_POS).encode())

    def run(self, x, max_sync=None):
        C = self.C
        x = np.ascontiguousarray(x, np.float32)
        cap = x.size // 3 + 8
        ms = max_sync or (x.size // 200 + 4)
        sym, rec, fl = np.zeros(cap, np.float32), np.zeros((cap, 4), np.int32), np.zeros(cap, np.uint8)
        pay = np.zeros((cap, 2), np.uint8)
        spos, spat = np.zeros(ms, np.int32), np.zeros(ms, np.uint8)
        pre, prel = np.zeros((ms, 90), np.uint8), np.zeros((ms, 90), np.uint8)
        thr = np.zeros((ms, 5), np.float32)
        ns = C.c_int(0)
        self.l.edrx_set_sync_thresholds(self.st, thr.ctypes.data, ms)
        k = self.l.edrx_run(self.st, x.ctypes.data, x.size, sym.ctypes.data, rec.ctypes.data, fl.ctypes.data, pay.ctypes.data, cap,
                            spos.ctypes.data, spat.ctypes.data, pre.ctypes.data, prel.ctypes.data, ms, C.byref(ns))
        assert k <= cap and ns.value <= ms
        n = ns.value
        return dict(sym=sym[:k].copy(), rec4=rec[:k].copy(), fl=fl[:k].copy(), pay=pay[:k].copy(), sync_pos=spos[:n].copy(),
                    sync_pat=spat[:n].copy(), pre=pre[:n].copy(), pre_rel=prel[:n].copy(), sync_thr=thr[:n].copy())

    def thresholds(self):
        t = np.zeros(7, np.float32)
        self.l.edrx_get_thresholds(self.st, t.ctypes.data)
        return t


def decode_stream(out, ea_mode=0, esk_mask=0):
    """every frame of one channel's loop output (LoopRx.run over the whole stream) -> list of decode_bits() dicts"""
    res = []
    for p, pat, t in zip(out["sync_pos"], out["sync_pat"], out["sync_thr"]):
        d = decode_slot(out["sym"], int(p), int(pat), t, ea_mode, esk_mask)
        if d["valid"]:
            res.append(d)
    return res
