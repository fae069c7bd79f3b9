"""dsd-neo_amd/csrc/ddn_p25h_rules.h compiled for the host (g++ -std=c++17, no GPU): the P25 Phase 1 handlers' decision rules against
the CPU oracle, never against the device code.  The status-counter functions exhaustively against a stepwise walk of the oracle's
block_take() rule (oracle/ddn_oracle_handlers.c) and the Python restatements of tests/shortcut_cases.py; the trellis tables against the
oracle's; and every rule against orc_p25h_symbol() inside the oracle's CQPSK loop, over traffic of every frame kind with NAC changes,
refused NACs and carrier losses: each oracle decision's words and carried state reproduced by the header's outcome functions, each
distance to the next decision or to the handler's return by its closed-form counts."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fecgen
import orc
import p25gen
import shortcut_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDLE, NID, BODY, TSBK, MPDU = range(5)          # orc_p25h.phase (P25H_*), and the header's PH_* - checked below
LEVEL = np.array([1.0, 3.0, -1.0, -3.0], np.float32)

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "ddn_p25h_rules.h"
using namespace ddn_p25h;
static_assert(PH_IDLE == 0 && PH_NID == 1 && PH_BODY == 2 && PH_TSBK == 3 && PH_MPDU == 4 && EV_NID == 1 && EV_TSBK == 2 && EV_MPDU == 3, "");
static_assert(deinterleave98(97) == 2 * (3 + 4 * 11) + 1 && half_rate_nibble(1) == 12 && body_symbols(0xF) == 159, "usable in constant expressions");
static std::string dir;
static void save(const std::string& name, const std::vector<int32_t>& v) {
    FILE* f = fopen((dir + "/" + name).c_str(), "wb");
    if (!f || fwrite(v.data(), 4, v.size(), f) != v.size()) { exit(3); }
    fclose(f);
}
int main(int, char** argv) {
    dir = argv[1];
    std::vector<int32_t> t;
    for (int i = 0; i < 98; i++) { t.push_back(deinterleave98(i)); }
    for (int i = 0; i < 16; i++) { t.push_back(half_rate_nibble(i)); }
    for (int i = 0; i < 16; i++) { t.push_back((int32_t)((half_rate_branches_by_nibble() >> (4 * i)) & 15u)); }
    for (int d = 0; d < 16; d++) { t.push_back(body_symbols(d)); }
    save("tables.i32", t);
    std::vector<int32_t> c; // [36][102][4] {status, data index, counter after n symbols, data among them}, then [36][2] a repetition
    for (int sk0 = 1; sk0 <= 36; sk0++) {
        for (int n = 0; n <= 101; n++) {
            int k = -1, nd = -1;
            c.push_back(block_is_status(sk0, n, k) ? 1 : 0);
            c.push_back(k);
            c.push_back(block_counter_after(sk0, n, nd));
            c.push_back(nd);
        }
    }
    for (int sk0 = 1; sk0 <= 36; sk0++) {
        int ska = -1;
        c.push_back(mpdu_block_symbols(sk0, ska));
        c.push_back(ska);
    }
    save("counter.i32", c);
    // decisions.i32 [n][10]: {kind, d0..d3, carried nac, p2_cc, block, end, status counter at the block's first symbol} -> out.i32 [n][20]
    FILE* f = fopen((dir + "/decisions.i32").c_str(), "rb");
    if (!f) { exit(2); }
    std::vector<int32_t> out;
    int32_t q[10];
    while (fread(q, 4, 10, f) == 10) {
        Event ev = {0, 0, 0, 0, 0, 0, 0};
        int nac = q[5], p2cc = q[6], phase = PH_IDLE, block = q[7], end = q[8], sk = q[9], ext = 0, more = 0, aux = 0, ska = 0;
        const int observed = observed_nac(nac, p2cc);
        if (q[0] == EV_NID) {
            const NidOutcome no = nid_outcome(q[1], q[2], q[3], q[4], nac, p2cc);
            nac = no.nac, p2cc = no.p2cc, ev = no.ev, aux = no.duid;
            const BlockPhase bp = block_phase_start(no.duid);
            phase = bp.phase;
            if (phase != PH_IDLE) {
                block = bp.block, end = bp.end, sk = bp.skipdibit;
                ext = phase == PH_TSBK ? TSBK_SYMBOLS : mpdu_block_symbols(sk, ska);
                more = 1;
            } else {
                ext = body_symbols(no.duid);
                phase = ext > 0 ? PH_BODY : PH_IDLE;
            }
        } else {
            const int crc_ok = q[4] & 1, sel = (q[4] >> 8) & 0xFF, nsym = q[0] == EV_TSBK ? TSBK_SYMBOLS : mpdu_block_symbols(sk, ska);
            int nd;
            sk = block_counter_after(sk, nsym, nd);
            if (q[0] == EV_MPDU && (nd != 98 || sk != ska)) { exit(4); } // the two closed forms of one repetition agree
            if (q[0] == EV_TSBK) {
                const TsbkOutcome to = tsbk_outcome((uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3], crc_ok, sel, block);
                if (tsbk_block_ends(block) && !to.last) { exit(5); }
                ev = to.ev, aux = to.last, block++;
                phase = to.last ? PH_IDLE : PH_TSBK;
                ext = to.last ? 0 : TSBK_SYMBOLS, more = to.last ? 0 : 1;
            } else {
                const HeaderOutcome ho = header_outcome((uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3], crc_ok, sel, end);
                ev = ho.ev, end = ho.end, aux = ho.end, block = 1;
                for (int bi = 1; bi < end; bi++) { // the remaining repetitions are read without a decision
                    ext += mpdu_block_symbols(sk, ska);
                    sk = ska;
                }
                phase = ext > 0 ? PH_MPDU : PH_IDLE;
            }
        }
        const int32_t row[20] = {ev.kind, ev.a, ev.b, ev.d0, ev.d1, ev.d2, ev.d3, nac, p2cc, phase, block, end, sk, ext, more, aux, observed, 0, 0, 0};
        out.insert(out.end(), row, row + 20);
    }
    fclose(f);
    save("out.i32", out);
    return 0;
}
'''


def _frames(rng, nac):
    """one round of every frame kind of test_rx_handlers_gpu._traffic"""
    f = [p25gen.make_frames(rng, 2, nac, crc=True, blocks=3)[0], p25gen.make_frames(rng, 2, nac, crc=True, blocks=1)[0],
         p25gen.make_frames(rng, 1, nac, crc=True, blocks=2)[0], p25gen.make_pdu(rng, nac, int(rng.integers(0, 5))),
         p25gen.make_pdu(rng, nac, 12, sap=61), p25gen.make_pdu(rng, nac, 3, good_crc=False),
         p25gen.frame_with_duid(rng, nac, [0x0, 0x3, 0xF, 0x5, 0xA][int(rng.integers(0, 5))], 339 + 30)]
    d = [0x3, 0xF, 0x5][int(rng.integers(0, 3))]
    f += [p25gen.frame_with_duid(rng, nac, d, {0x3: 15, 0xF: 159, 0x5: 807}[d] + 3), p25gen.frame_with_duid(rng, nac, 0x9, 40)]
    return [f[k] for k in rng.permutation(len(f))]


def _stream(seed, body_noise):
    """the dibits of one channel: rounds of every frame kind under changing NACs - a new one, 0 and 0xFFF (refused), the first again -
    a carrier loss (1900 symbols without a sync: the loop's 1800-symbol timeout) ahead of some rounds, so that their first NID is
    decoded with p2_cc as the observed NAC; a blank NID (fails) and a TSDU whose third block carries no last-block flag.  Frame syncs
    and NIDs at a noise of 0.2 of the inner level, what follows them in every other frame at body_noise (the list decoder's cases)"""
    rng = np.random.default_rng(seed)
    parts, loud = [rng.integers(0, 4, 40)], []
    for k, nac in enumerate([0x293, 0x123, 0x000, 0x123, 0xFFF, 0x293, 0x4A5, 0x4A5, 0xFFF, 0x001, 0x000, 0xFFE]):
        if k in (1, 5, 6, 9):
            parts.append(rng.integers(0, 4, 1900))
        for j, fr in enumerate(_frames(rng, nac)):
            at = sum(len(q) for q in parts)
            loud += [(at + 57, at + len(fr))] * (j & 1)
            parts += [np.asarray(fr) & 3, rng.integers(0, 4, int(rng.integers(5, 40)))]
        bad = p25gen.frame_with_duid(rng, nac, 0x3, 20)
        bad[24:57] = rng.integers(0, 4, 33)
        noflag = shortcut_cases.tsdu(rng, [True] * 4, nac)[0]            # (four blocks, the flag on the fourth: three are read)
        parts += [bad & 3, rng.integers(0, 4, 30), noflag & 3, rng.integers(0, 4, 20)]
    d = np.concatenate(parts + [rng.integers(0, 4, 900)])
    sigma = np.full(len(d), 0.2)
    for a, b in loud:
        sigma[a:b] = body_noise
    return (LEVEL[d] + sigma * rng.standard_normal(len(d))).astype(np.float32)


def _oracle_run(sym):
    """the oracle's CQPSK loop symbol by symbol -> (event rows, event data, handler words [n][8] after every symbol:
    phase, block, end, skipdibit, nac, p2_cc, idx, k)"""
    rx = orc.OracleCqRx(orc.CQ_P25P1, -1)
    o = C.CDLL(orc.ORACLE_SO)         # (a handle of its own: the prototypes set below stay out of the shared one)
    o.orc_cqrx_symbol.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    o.orc_cqrx_get_handler.argtypes = [C.c_void_p, C.c_void_p]
    words = np.zeros((len(sym), 8), np.int32)
    rec4 = (C.c_int * 4)()
    for i, x in enumerate(sym):
        o.orc_cqrx_symbol(rx.st, float(x), rec4)
        o.orc_cqrx_get_handler(rx.st, words[i].ctypes.data)
    assert rx.events.n <= 4096
    return rx.events.rows(), rx.events.data(), words


@pytest.fixture(scope="module")
def run():
    """-> the program's tables, and per stream (events, data, handler words, out [n][20])"""
    streams = [_oracle_run(_stream(11 + k, noise)) for k, noise in enumerate((0.2, 0.6, 0.8))]
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(SRC)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "dsd-neo_amd", "csrc"),
                               os.path.join(d, "t.cpp"), "-o", exe])
        outs = []
        for rows, data, words in streams:
            dec, sk = [], 22
            for (pos, kind, a, b, c), d4 in zip(rows, data):
                before = words[pos - 1]
                if kind == orc.HEV_P25_NID:
                    sk = 22
                dec.append([kind] + [int(v) for v in d4] + [int(before[4]), int(before[5]), int(before[1]), int(before[2]), sk])
                sk = int(words[pos][3])     # (the oracle's own counter: the next block's start)
            np.array(dec, np.int32).tofile(os.path.join(d, "decisions.i32"))
            subprocess.check_call([exe, d])
            outs.append(np.fromfile(os.path.join(d, "out.i32"), np.int32).reshape(-1, 20))
        tables = np.fromfile(os.path.join(d, "tables.i32"), np.int32)
        counter = np.fromfile(os.path.join(d, "counter.i32"), np.int32)
    return tables, counter, [s + (o,) for s, o in zip(streams, outs)]


def _walk(sk0, n):
    """block_take() of oracle/ddn_oracle_handlers.c over n symbols from the counter at sk0 -> (is symbol i a status symbol, data dibits
    before symbol i) for i < n, the counter and the data count afterwards"""
    sk, k, status, index = sk0, 0, [], []
    for _ in range(n):
        index.append(k)
        if sk // 36 == 0:
            k += 1
            status.append(0)
        else:
            sk = 0
            status.append(1)
        sk += 1
    return status, index, sk, k


def test_status_counter_functions_equal_the_stepwise_walk(run):
    """every starting counter 1..36, every symbol count 0..101: block_is_status / block_counter_after against the walk;
    mpdu_block_symbols against the walk stopped at the 98th data dibit (at most 101 symbols) and against shortcut_cases"""
    c = run[1]
    tab, rep = c[:36 * 102 * 4].reshape(36, 102, 4), c[36 * 102 * 4:].reshape(36, 2)
    for sk0 in range(1, 37):
        status, index, _, _ = _walk(sk0, 102)
        assert list(tab[sk0 - 1, :, 0]) == status and list(tab[sk0 - 1, :, 1]) == index, sk0
        for n in range(102):
            _, _, sk, k = _walk(sk0, n)
            assert (tab[sk0 - 1, n, 2], tab[sk0 - 1, n, 3]) == (sk, k), (sk0, n)
        n = next((n for n in range(1, 102) if _walk(sk0, n)[3] == 98), 101)
        assert (rep[sk0 - 1, 0], rep[sk0 - 1, 1]) == (n, _walk(sk0, n)[2]), sk0
        assert shortcut_cases.mpdu_block_symbols(sk0) == n
        data = shortcut_cases.block_data_symbols(sk0, 102)          # what classify_block takes for a block's data dibits
        assert data == [s for s in range(102) if not tab[sk0 - 1, s, 0]] and [int(tab[sk0 - 1, s, 1]) for s in data] == list(range(len(data))), sk0
        assert all(tab[sk0 - 1, n, 3] == sum(s < n for s in data) for n in range(102)), sk0       # block_counter_after's data count


def test_trellis_tables_equal_the_oracle(run):
    t = run[0]
    dei, nib, inv, body = t[:98], t[98:114], t[114:130], t[130:146]
    o = fecgen.tables()
    assert sorted(dei) == list(range(98))
    assert np.array_equal(dei, o["il"].astype(np.int32))          # transmit position i carries de-interleaved dibit il[i]
    assert [shortcut_cases.deinterleave98(i) for i in range(98)] == list(dei)
    assert np.array_equal(nib, o["half"].astype(np.int32))
    assert all(nib[inv[v]] == v for v in range(16))
    assert list(body) == [339, 0, 0, 15, 0, 807, 0, 0, 0, 0, 807, 0, 0, 0, 0, 159]   # body_symbols() of ddn_oracle_handlers.c


def test_every_oracle_decision_is_reproduced(run):
    """words, data, carried NAC pair, phase / block / end / status counter after the decision, and the distance to what follows"""
    seen = dict(nac_update=0, refused_0=0, refused_fff=0, p2cc_observed=0, failed=0, last_flag=0, third_block=0,
                third_no_flag=0, list_other=0, hdr_bad=0, sap_cap=0, blks=set(), duid=set(), frames=0)
    for rows, data, words, out in run[2]:
        assert len(out) == len(rows) > 150
        ev_pos = [r[0] for r in rows]
        idle = np.flatnonzero(words[:, 0] == IDLE)
        for j, ((pos, kind, a, b, c), d4, g) in enumerate(zip(rows, data, out)):
            before, after = words[pos - 1], words[pos]
            tag = (pos, kind, a, b, c, list(d4), list(g))
            assert g[0] == kind and g[1] == a and (g[2] & 0xFFFF) == (b & 0xFFFF) and ((g[2] >> 16) & 0xFFFF) == (c & 0xFFFF), tag
            assert np.array_equal(g[3:7], d4), tag
            assert (g[7], g[8]) == (after[4], after[5]), tag                       # the carried NAC pair
            assert g[9] == after[0], tag                                           # the phase that follows
            nac, p2 = int(before[4]), int(before[5])
            valid = lambda v: v > 0 and v <= 0xFFF and v != 0xFFF                  # nac_valid_observed() of ddn_oracle_handlers.c
            assert g[16] == (nac if valid(nac) else (p2 if valid(p2) else 0)), tag
            if kind == orc.HEV_P25_NID:
                seen["frames"] += 1
                assert g[15] == (c & 0xFF), tag                                    # effective DUID, 0xFF on failure
                if g[9] in (TSBK, MPDU):
                    assert tuple(g[10:13]) == tuple(after[1:4]) and after[6] == 0 and after[7] == 0, tag
                if a > 0:
                    seen["duid"].add(int(c & 0xFF))
                    seen["nac_update"] += int(after[4] != nac)
                    seen["refused_0"] += int(b == 0 and nac != 0 and after[4] == nac)
                    seen["refused_fff"] += int((b & 0xFFF) == 0xFFF and nac != 0xFFF and after[4] == nac)
                else:                       # (a NID that fails, or spells an undefined DUID: the decoder refuses both)
                    seen["failed"] += int(g[13] == 0 and after[0] == IDLE)
                seen["p2cc_observed"] += int(nac == 0 and valid(p2))
            elif kind == orc.HEV_P25_TSBK:
                assert (g[10], g[12]) == (after[1], after[3]) and g[15] == int(after[0] == IDLE), tag
                flag = (c >> 8) & 1
                seen["last_flag"] += int(flag and a < 2)
                seen["third_block"] += int(a == 2)
                seen["third_no_flag"] += int(a == 2 and not flag)
                seen["list_other"] += int((c & 0xFF) > 0)
            else:
                assert g[11] == after[2] == g[15] and (g[13] > 0) == (after[2] > 1), tag
                seen["hdr_bad"] += int(a == 0)
                seen["list_other"] += int(((int(d4[3]) >> 8) & 0xFF) > 0)
                if a:
                    sap, blks = (int(d4[0]) >> 8) & 0x3F, (int(d4[1]) >> 16) & 0x7F
                    seen["sap_cap"] += int(sap in (61, 63) and blks > 10 and after[2] == 4)
                    seen["blks"].add(blks)
            # the distance: another decision falls due after g[13] symbols (g[14]), or the handler returns with the last of them
            ext, more = int(g[13]), int(g[14])
            assert pos + ext < len(words), tag
            if more:
                assert ev_pos[j + 1] == pos + ext and not np.any(words[pos:pos + ext, 0] == IDLE), tag
            else:
                assert idle[np.searchsorted(idle, pos)] == pos + ext, tag
                assert j + 1 == len(rows) or ev_pos[j + 1] > pos + ext, tag
    assert seen["frames"] >= 300, seen
    assert seen["duid"] >= {0x0, 0x3, 0x5, 0x7, 0xC, 0xF} and 12 in seen["blks"] and len(seen["blks"]) >= 4, seen
    for k, v in seen.items():
        assert v, (k, seen)
