"""Synthetic DMR data PDUs for the PDU tests, built on tests/dmrgen.py: data headers of every format, block sequences of every rate
with their CRC9 / CRC32 / CRC16, padding and the DBSN order, multi-block control messages, unified data transport with a fixed and
with a reserved block count.  TEST INFRASTRUCTURE - the product never imports this.

A plan is a list of items dict(slot, type, one of bits96 / bytes18 / info196, ...) in air order.  fec_bursts() turns it into the
FEC-level dicts tests/dmr_pdu.py walks (what ddn_dmr_data.hip delivers for a cleanly received burst); air_dibits() into the dibits
dmrgen.burst() puts on the air.  The CRCs are computed here on their own, not with the restatement's helpers."""
import numpy as np

import dmrgen
import p25gen
import rx4

BLOCK_LEN = {(7, 0): 12, (8, 0): 18, (10, 0): 24, (7, 1): 10, (8, 1): 16, (10, 1): 22}
CRC9_MASK = {7: 0x0F0, 8: 0x1FF, 10: 0x10F}


def _bits(v, n):
    return [(int(v) >> (n - 1 - i)) & 1 for i in range(n)]


def _byte_bits(by):
    return [int(x) for x in np.unpackbits(np.asarray(by, np.uint8))]


def _ccitt(bits):
    return rx4.crc_ccitt_bits(bits) ^ 0xFFFF


def crc32_trailer(body):
    """the four bytes that close a PDU of `body` (an even number of bytes): CRC-32 (0x04C11DB7, initial value 0, no reflection) over the
    bytes taken in swapped pairs, sent least significant byte first"""
    assert len(body) % 2 == 0
    crc = 0
    for i in range(len(body)):
        crc ^= int(body[i ^ 1]) << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return [crc & 0xFF, (crc >> 8) & 0xFF, (crc >> 16) & 0xFF, crc >> 24]


def _with_ccitt(bits80, mask, good=True):
    c = (_ccitt(bits80) ^ mask ^ (0 if good else 0x0100)) & 0xFFFF
    return np.array(list(bits80) + _bits(c, 16), np.uint8)


def header(slot, dpf, blocks, sap=4, gi=0, a=0, poc=0, tgt=0x000102, src=0x0A0B0C, good_crc=True, errs=0):
    """a data header (type 6) of format 2 (unconfirmed), 3 (confirmed), 1 (response), 13 / 14 (short data: `blocks` = appended blocks)"""
    if dpf in (13, 14):
        b0 = (gi << 7) | (a << 6) | (((blocks >> 4) & 3) << 4) | dpf
        b1 = (sap << 4) | (blocks & 0xF)
        b8, b9 = 0, 0
    else:
        b0 = (gi << 7) | (a << 6) | (((poc >> 4) & 1) << 4) | dpf
        b1 = (sap << 4) | (poc & 0xF)
        b8, b9 = 0x80 | (blocks & 0x7F), 0
    by = [b0, b1, tgt >> 16, (tgt >> 8) & 0xFF, tgt & 0xFF, src >> 16, (src >> 8) & 0xFF, src & 0xFF, b8, b9]
    return dict(slot=slot, type=6, bits96=_with_ccitt(_byte_bits(by), 0xCCCC, good_crc), errs=errs)


def udt_header(slot, appended, udt_format=0, pf=0, gi=0, tgt=0x000203, src=0x0B0C0D):
    """a UDT header (format 0): `appended` blocks follow (1 .. 4); udt_format 5 with appended = 3 is the reserved count"""
    by = [(gi << 7), udt_format & 0xF, tgt >> 16, (tgt >> 8) & 0xFF, tgt & 0xFF, src >> 16, (src >> 8) & 0xFF, src & 0xFF,
          (appended - 1) & 3, (pf << 6) | 0x0A]
    return dict(slot=slot, type=6, bits96=_with_ccitt(_byte_bits(by), 0xCCCC))


def proprietary_header(slot, rng, mnis=True):
    """a proprietary header (format 15): SAP 1 / MFID 0x10 is the MNIS header whose ten bytes open the PDU, any other takes a block off
    the count"""
    by = [0x1F, 0x10] if mnis else [0x4F, 0x77]
    by += [int(x) for x in rng.integers(0, 256, 8)]
    return dict(slot=slot, type=6, bits96=_with_ccitt(_byte_bits(by), 0xCCCC))


def block(slot, rate, confirmed, chunk, dbsn=0, good_crc9=True):
    """one block of rate 7 (1/2), 8 (3/4) or 10 (1) carrying `chunk` (BLOCK_LEN bytes)"""
    chunk = [int(x) for x in chunk]
    assert len(chunk) == BLOCK_LEN[(rate, int(confirmed))]
    if not confirmed:
        if rate == 7:
            return dict(slot=slot, type=7, bits96=np.array(_byte_bits(chunk), np.uint8))
        if rate == 8:
            return dict(slot=slot, type=8, bytes18=np.array(chunk, np.uint8))
        info = np.zeros(196, np.uint8)
        info[0:96], info[100:196] = _byte_bits(chunk[:12]), _byte_bits(chunk[12:])
        return dict(slot=slot, type=10, info196=info)
    c = p25gen.crc9(_byte_bits(chunk) + _bits(dbsn, 7)) ^ CRC9_MASK[rate] ^ (0 if good_crc9 else 0x005)
    head = _bits(dbsn, 7) + _bits(c, 9)
    if rate == 7:
        return dict(slot=slot, type=7, bits96=np.array(head + _byte_bits(chunk), np.uint8))
    if rate == 8:
        return dict(slot=slot, type=8, bytes18=np.packbits(np.array(head + _byte_bits(chunk), np.uint8)))
    info = np.zeros(196, np.uint8)
    info[0:16], info[16:96], info[100:196] = head, _byte_bits(chunk[:10]), _byte_bits(chunk[10:])
    return dict(slot=slot, type=10, info196=info)


def data_pdu(rng, slot, rate, confirmed, n_blocks, good_crc32=True, dbsn0=0, lead=(), **hdr):
    """header + n_blocks blocks whose payload closes with the CRC32 -> (items, the row the PDU should complete with).  `lead`: bytes
    that already open the row (the MNIS header's ten) and take part in the CRC32"""
    blen = BLOCK_LEN[(rate, int(confirmed))]
    total = n_blocks * blen
    body = [int(x) for x in rng.integers(0, 256, total - 4)]
    tr = crc32_trailer(list(lead) + body)
    if not good_crc32:
        tr[1] ^= 0x40
    row = body + tr
    items = [header(slot, 3 if confirmed else 2, n_blocks, **hdr)]
    for k in range(n_blocks):
        items.append(block(slot, rate, confirmed, row[k * blen:(k + 1) * blen], dbsn=(dbsn0 + k) & 0x7F))
    return items, np.array(list(lead) + row, np.uint8)


def mbc(rng, slot, n_cont, good_crc16=True, good_header=True):
    """an MBC header (type 4) and n_cont continuation blocks (type 5), the last with LB set and the CRC16 over the continuation blocks"""
    hb = [int(x) for x in rng.integers(0, 256, 10)]
    hb[0] &= 0x3F                                              # LB = 0, PF = 0
    items = [dict(slot=slot, type=4, bits96=_with_ccitt(_byte_bits(hb), 0xAAAA, good_header))]
    cont = [int(x) for x in rng.integers(0, 256, 12 * n_cont - 2)]
    for k in range(n_cont):
        cont[12 * k] = (cont[12 * k] & 0x3F) | (0x80 if k == n_cont - 1 else 0)
    c = _ccitt(_byte_bits(cont)) ^ (0 if good_crc16 else 0x0011)
    cont += [c >> 8, c & 0xFF]
    for k in range(n_cont):
        items.append(dict(slot=slot, type=5, bits96=np.array(_byte_bits(cont[12 * k:12 * k + 12]), np.uint8)))
    return items


def udt(rng, slot, appended, reserved=False, good_crc16=True):
    """a UDT header and its appended rate 1/2 blocks, the last closing with the CRC16 over them; reserved: the header names the
    reserved count (format 5, three blocks) and the message ends after `appended` blocks, where the CRC16 checks"""
    items = [udt_header(slot, 3, udt_format=5) if reserved else udt_header(slot, appended)]
    body = [int(x) for x in rng.integers(0, 256, 12 * appended - 2)]
    c = _ccitt(_byte_bits(body)) ^ (0 if good_crc16 else 0x0101)
    body += [c >> 8, c & 0xFF]
    for k in range(appended):
        items.append(dict(slot=slot, type=7, bits96=np.array(_byte_bits(body[12 * k:12 * k + 12]), np.uint8)))
    return items


def other(rng, slot, ty):
    """a burst of a type the assembler does not take: PI 0, VLC 1, TLC 2, CSBK 3, idle 9, USBD 11"""
    if ty == 9:
        return dict(slot=slot, type=9, bits96=rng.integers(0, 2, 96).astype(np.uint8))
    return dict(slot=slot, type=ty, bits96=dmrgen.payload_bits(ty, rng))


def terminator(slot):
    """a readable data terminator: TLC with FLCO 0x30"""
    d = [0x30, 0, 0, 0, 1, 0, 0, 2, 0]
    p = dmrgen.rs_12_9_parity(d)
    m = dmrgen.CRC_MASK[2]
    return dict(slot=slot, type=2, bits96=np.array(_byte_bits(d + [p[0] ^ (m >> 16), p[1] ^ ((m >> 8) & 0xFF), p[2] ^ (m & 0xFF)]), np.uint8))


def interleave(a, b):
    """two time slots' items, alternating while both last"""
    out = []
    for k in range(max(len(a), len(b))):
        out += a[k:k + 1] + b[k:k + 1]
    return out


# ---- FEC level -----------------------------------------------------------------------------------------------------------------------
def fec_burst(it):
    """what the data-burst stage delivers for the item received cleanly (tests/dmr_data.data_burst()'s fields + the slot)"""
    ty = it["type"]
    out = dict(slot=it["slot"], type=ty, errs=int(it.get("errs", 0)), crc=0, bytes12=np.zeros(12, np.uint8), info=np.zeros(196, np.uint8),
               unconfirmed=np.zeros(18, np.uint8), pool=[])
    if ty == 8:
        b = np.asarray(it["bytes18"], np.uint8)
        bits = np.unpackbits(b)
        ok = int(p25gen.crc9(list(bits[16:144]) + list(bits[:7])) == (rx4.bits_int(bits[7:16]) ^ 0x1FF))
        out.update(crc=1, unconfirmed=b.copy(), pool=it.get("pool", [(b.copy(), 0, ok, int(b[0]) >> 1)]))
    elif ty == 10:
        info = np.asarray(it["info196"], np.uint8)
        out.update(info=info.copy(), crc=1 | (2 if dmrgen.crc9_confirmed_rate1(info) == rx4.bits_int(info[7:16]) else 0))
    else:
        b = np.asarray(it["bits96"], np.uint8)
        out["bytes12"] = np.packbits(b)
        if ty in (1, 2):
            out["crc"] = int(it.get("rs_ok", 1))
        elif ty == 7:
            out["crc"] = 1 | (2 if p25gen.crc9(list(b[16:96]) + list(b[:7])) == (rx4.bits_int(b[7:16]) ^ 0x0F0) else 0)
        elif ty != 9 and ty <= 11:
            n = 0 if ty == 5 else 16
            ext = (rx4.bits_int(b[96 - n:]) if n else 0) ^ dmrgen.CRC_MASK.get(ty, 0)
            out["crc"] = int(_ccitt(b[:80]) == ext)
    return out


def fec_bursts(items):
    return [fec_burst(it) for it in items]


# ---- the traffic plan -----------------------------------------------------------------------------------------------------------------
def traffic(seed=0):
    """one channel's bursts with every case the PDU tests hold to floors -> (items, marks [(before, kind)], notes: name -> index of the
    item that matters).  Both time slots carry different PDUs side by side; the marks are where a test of the walk alone puts
    dmr_reset_blocks() (kind 0) and carrier loss (kind 1)."""
    rng = np.random.default_rng(seed)
    items, marks, notes = [], [], {}

    def add(name, seq):
        notes[name] = len(items) + len(seq) - 1
        items.extend(seq)

    add("unconf12|conf34", interleave(data_pdu(rng, 0, 7, False, 3)[0], data_pdu(rng, 1, 8, True, 4, dbsn0=5)[0]))
    add("conf12|conf1", interleave(data_pdu(rng, 0, 7, True, 3)[0], data_pdu(rng, 1, 10, True, 2, dbsn0=126)[0]))
    add("unconf34|unconf1", interleave(data_pdu(rng, 0, 8, False, 2, poc=7)[0], data_pdu(rng, 1, 10, False, 2)[0]))
    # the MNIS header: ten of its bytes open the row, the blocks count from 2
    p = proprietary_header(0, rng)
    lead = np.packbits(p["bits96"])[:10]
    d, _ = data_pdu(rng, 0, 7, False, 3, lead=[int(x) for x in lead])
    add("mnis|mbc", interleave([header(0, 2, 4), p] + d[1:], mbc(rng, 1, 2)))
    p = proprietary_header(1, rng, mnis=False)
    d, _ = data_pdu(rng, 1, 8, False, 3)
    add("udt|vertex", interleave(udt(rng, 0, 2), [header(1, 2, 4), p] + d[1:]))
    add("udt_reserved|mbc3", interleave(udt(rng, 0, 2, reserved=True), mbc(rng, 1, 3)))
    add("bad_crc32|bad_crc16", interleave(data_pdu(rng, 0, 7, False, 2, good_crc32=False)[0], mbc(rng, 1, 1, good_crc16=False)))
    # a header rejected for its CRC: the blocks behind it meet the initial state
    add("header_crc", [header(0, 2, 2, good_crc=False)] + data_pdu(rng, 0, 7, False, 2)[0][1:])
    add("header_fec", [header(1, 3, 2, errs=1)])
    # a DBSN sequence error in mid-PDU: block 2 of 4 arrives as DBSN 9
    d, _ = data_pdu(rng, 0, 8, True, 4, dbsn0=3)
    d[3] = block(0, 8, True, rng.integers(0, 256, 16), dbsn=9)
    add("seq_error", d)
    # a bad CRC9 leaves the expectation alone
    d, _ = data_pdu(rng, 1, 7, True, 3)
    d[2] = block(1, 7, True, rng.integers(0, 256, 10), dbsn=1, good_crc9=False)
    add("bad_crc9", d)
    # resets in mid-PDU: a slot-type failure (dmr_reset_blocks()), then carrier loss; the PDU behind each completes
    d, _ = data_pdu(rng, 0, 7, False, 3)
    add("reset_mid", d[:2])
    marks.append((len(items), 0))
    add("after_reset", d[2:] + data_pdu(rng, 0, 7, False, 2)[0])
    d, _ = data_pdu(rng, 1, 10, True, 3)
    add("loss_mid", d[:2])
    marks.append((len(items), 1))
    add("after_loss", d[2:] + data_pdu(rng, 1, 8, True, 2)[0])
    # a terminator in mid-PDU, the other types in between, a short-data header
    d, _ = data_pdu(rng, 0, 7, False, 3)
    add("terminated", d[:2] + [terminator(0)] + d[2:])
    add("others", [other(rng, k & 1, ty) for k, ty in enumerate((0, 1, 3, 9, 11, 2))])
    d, _ = data_pdu(rng, 1, 7, True, 2)
    add("short_data", [header(1, 13, 2, sap=10, a=1)] + d[1:])
    return items, marks, notes


# ---- on the air -----------------------------------------------------------------------------------------------------------------------
GAP = 2000          # symbols without a sync: past the loop's 1800-symbol carrier-loss count


def air_plan(seed=0):
    """a shorter plan for the tests that go through the receive loop: CSBKs until the colour-code gate locks, PDUs of every rate on both
    time slots, MBCs of two and three blocks, a UDT message with a fixed block count and a CRC-terminated one, a DBSN sequence error, a PDU cut by a burst whose slot type fails, one cut by a
    gap without carrier (dict(gap=symbols)), a PDU behind each -> items"""
    rng = np.random.default_rng(100 + seed)
    csbk = lambda n: [other(rng, k & 1, 3) for k in range(n)]
    items = csbk(8)
    items += interleave(data_pdu(rng, 0, 7, False, 3)[0], data_pdu(rng, 1, 8, True, 3, dbsn0=5)[0])
    items += interleave(data_pdu(rng, 0, 10, True, 2, dbsn0=127)[0], mbc(rng, 1, 2))
    items += interleave(udt(rng, 0, 2, reserved=True), data_pdu(rng, 1, 7, True, 2, good_crc32=False)[0])
    items += interleave(udt(rng, 0, 2), mbc(rng, 1, 3))
    d, _ = data_pdu(rng, 0, 8, True, 3, dbsn0=3)
    d[2] = block(0, 8, True, rng.integers(0, 256, 16), dbsn=9)
    items += d
    d, _ = data_pdu(rng, 1, 7, False, 3)
    hurt = other(rng, 0, 3)
    hurt["hurt_slot_type"] = True
    items += d[:2] + [hurt] + d[2:] + data_pdu(rng, 1, 7, False, 2)[0]
    d, _ = data_pdu(rng, 0, 10, True, 3)
    items += d[:2] + [dict(gap=GAP)] + csbk(8) + d[2:] + data_pdu(rng, 0, 8, True, 2)[0]
    p = proprietary_header(1, rng)
    d, _ = data_pdu(rng, 1, 7, False, 2, lead=[int(x) for x in np.packbits(p["bits96"])[:10]])
    items += [header(1, 2, 3), p] + d[1:] + [header(0, 2, 2, good_crc=False)] + csbk(2)
    return items


def air_dibits(items, cc=7, seed=0):
    """the items as BS data bursts back to back; an item with hurt_slot_type = True has its slot type broken past Golay(20,8); a gap is
    that many random dibits"""
    out = []
    rng = np.random.default_rng(seed)
    for it in items:
        if "gap" in it:
            out.append(rng.integers(0, 4, it["gap"]).astype(np.int8))
            continue
        if "bytes18" in it:
            info = dmrgen.r34_info(it["bytes18"])
        elif "info196" in it:
            info = it["info196"]
        else:
            info = dmrgen.bptc_196x96(it["bits96"])
        d = dmrgen.burst(it["slot"], cc, it["type"], info)
        if it.get("hurt_slot_type"):
            d = d.copy()
            d[61:66] ^= np.array([3, 1, 2, 3, 0], np.int8)
            d[90:95] ^= np.array([0, 2, 1, 0, 3], np.int8)
        out.append(d)
    return np.concatenate(out)


_air = {}


def air_batch():
    """air_plan(0) as cu8 I/Q of three channels: as sent, delayed, and starting 2011 samples later (chain_fsk4_stream._batch) ->
    [3][L][2]; L is a multiple of 6000"""
    if "x" not in _air:
        import chain_fsk4_stream as cs
        dib = air_dibits(air_plan(0))
        L = -(-(10 * len(dib) + 3000) // 6000) * 6000
        iq = p25gen.modulate_cu8(dib, L + 2011, lead=300, seed=4, noise=0.02)
        _air["x"] = cs._batch(iq, L, 1234, later=2011)
    return _air["x"]
