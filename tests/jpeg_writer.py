"""A baseline JPEG writer for tests (numpy only, no Pillow): files are built from quantised coefficients the caller supplies per
component and block, so there is no forward DCT and every header and entropy-coding choice another encoder might make is the
caller's: table ids and precisions, SOF0 / SOF1, sampling bytes, component ids, the restart interval, extra and repeated segments,
fill bytes, pad bits, bytes after EOI.  write() also returns where every block and every RSTn marker starts in the file, which is
what the window cases of tools/gen_jpeg_golden_foreign.py are built from (docs/design/ingest.md, "What the tests pin")."""
import numpy as np


def _canonical(counts, symbols):
    """(16 counts, symbols) -> {symbol: (code, length)}, the canonical code of a DHT segment."""
    assert len(counts) == 16 and sum(counts) == len(symbols) and len(set(symbols)) == len(symbols)
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            assert code < (1 << l) - 1, "the all-ones code is not allowed"
            out[symbols[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


# Default tables: DC categories 0 .. 11, and an AC table that holds every (run, size) with size 1 .. 10, EOB and ZRL.  Their counts are
# those of the typical tables of the standard's Annex K; the symbol order is by rising run and size after the most frequent ones.
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
_AC_ALL = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
_AC_FIRST = [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
             0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0]
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC_FIRST + sorted(set(_AC_ALL) - set(_AC_FIRST)))
_AC_FIRST_C = [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
               0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0]
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC_FIRST_C + sorted(set(_AC_ALL) - set(_AC_FIRST_C)))
FLAT_QUANT = [8] * 64


def segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def jfif():
    return segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")


def adobe(transform):
    return segment(0xEE, b"Adobe\0\x64\x00\x00\x00\x00" + bytes([transform]))


def com(n):
    """A comment segment of n bytes in all (n >= 4): shifts everything behind it by n."""
    assert n >= 4
    return segment(0xFE, bytes(0x41 + k % 26 for k in range(n - 4)))


def dri(interval):
    return segment(0xDD, int(interval).to_bytes(2, "big"))


def dqt(*tables):
    """tables: (id, 64 entries in zigzag order, sixteen_bit) each; one segment."""
    body = b""
    for tq, entries, wide in tables:
        assert len(entries) == 64 and 0 <= tq <= 3
        body += bytes([(0x10 if wide else 0) | tq]) + b"".join(int(v).to_bytes(2 if wide else 1, "big") for v in entries)
    return segment(0xDB, body)


def dht(*tables):
    """tables: (class 0 DC / 1 AC, id, (16 counts, symbols)) each; one segment."""
    body = b""
    for tc, th, (counts, symbols) in tables:
        _canonical(counts, symbols)
        body += bytes([(tc << 4) | th]) + bytes(counts) + bytes(symbols)
    return segment(0xC4, body)


class _Bits:
    """The entropy-coded bytes of a scan: bits first in first out, a zero byte stuffed behind every 0xFF."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, length):
        assert 0 <= value < (1 << length)
        self.acc, self.n = (self.acc << length) | value, self.n + length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self, ones):
        if self.n:
            k = 8 - self.n
            self.put((1 << k) - 1 if ones else 0, k)


def _category(v):
    return int(abs(int(v))).bit_length()


def _put_value(bits, v, s):
    if s:
        bits.put(int(v) if v > 0 else int(v) + (1 << s) - 1, s)


def _put_block(bits, zz, pred, dc, ac):
    """One block (64 quantised coefficients in zigzag order): DC difference, then (run, size) pairs with ZRL for runs of 16 and an EOB
    unless the last coefficient is at index 63."""
    diff = int(zz[0]) - pred
    s = _category(diff)
    bits.put(*dc[s])
    _put_value(bits, diff, s)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
        s = _category(v)
        bits.put(*ac[(run << 4) | s])
        _put_value(bits, v, s)
        run = 0
    if run:
        bits.put(*ac[0x00])
    return int(zz[0])


class Written:
    """write()'s result: .data, the file; .scan_off, the first byte of the scan; .scan_end, the offset of the EOI marker (of the first
    of its fill bytes); .block_off[i], the file offset of the byte that holds the first bit of block i (blocks in scan order);
    .rst_off[k], the offset of the 0xFF of restart marker k (behind its fill bytes); .mcus, .blocks_per_mcu."""


def write(w, h, coefs, sampling=(1, 1), sof=0xC0, quant=None, quant16=(), huff=None, comp_ids=None, comp_quant=None, comp_huff=None,
          gray_factors=0x11, restart=None, pre_sof=(), pre_sos=(), layout=None, dht_merged=False, eoi_fill=0, rst_fill=None,
          rst_number=None, pad_ones=True, trailer=b""):
    """coefs: one int array per component, [block rows, block columns, 64] in zigzag order, over whole MCUs (luma sampling[0] x
    sampling[1] blocks per MCU when there are three components; chroma is 1x1).
    quant {id: 64 zigzag entries}, ids in quant16 written with 16-bit entries; huff {(class, id): (counts, symbols)};
    comp_ids, comp_quant (table id per component), comp_huff ((dc id, ac id) per component); gray_factors: the sampling byte of a
    one-component frame (the scan is one block per MCU whatever it says); restart: None for no DRI, else the interval (0 included:
    then no markers are written; an interval of at least the MCU count likewise).
    layout: the segments between SOI and the scan, a list of "DQT", "SOF", "DHT", "DRI", "SOS" and raw bytes (segment(), jfif(),
    adobe(), com(), dri(), dqt(), dht(), or b"\\xff" fill bytes before the next marker); default: pre_sof, DQT, SOF, DHT, DRI, pre_sos,
    SOS.  dht_merged: all Huffman tables in one DHT segment.  eoi_fill: 0xFF fill bytes before EOI.  rst_fill {k: n}: fill bytes before
    restart marker k; rst_number {k: m}: marker k written as RSTm.  pad_ones: the pad bits before a marker."""
    nc = len(coefs)
    assert nc in (1, 3)
    hs, vs = sampling if nc == 3 else (1, 1)
    quant = {0: FLAT_QUANT, 1: FLAT_QUANT} if quant is None else quant
    huff = {(0, 0): DC_LUMA, (1, 0): AC_LUMA, (0, 1): DC_CHROMA, (1, 1): AC_CHROMA} if huff is None else huff
    comp_ids = [1, 2, 3][:nc] if comp_ids is None else comp_ids
    comp_quant = [0, 1, 1][:nc] if comp_quant is None else comp_quant
    comp_huff = [(0, 0), (1, 1), (1, 1)][:nc] if comp_huff is None else comp_huff
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    coefs = [np.asarray(c) for c in coefs]
    assert coefs[0].shape == (my * vs, mx * hs, 64) and all(c.shape == (my, mx, 64) for c in coefs[1:]), [c.shape for c in coefs]

    factors = [gray_factors] if nc == 1 else [(hs << 4) | vs, 0x11, 0x11]
    seg = {
        "DQT": b"".join(dqt((t, quant[t], t in quant16)) for t in sorted(quant)),
        "SOF": segment(sof, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) +
                       b"".join(bytes([comp_ids[c], factors[c], comp_quant[c]]) for c in range(nc))),
        "DHT": dht(*[(tc, th, huff[(tc, th)]) for tc, th in sorted(huff)]) if dht_merged else
               b"".join(dht((tc, th, huff[(tc, th)])) for tc, th in sorted(huff)),
        "DRI": b"" if restart is None else dri(restart),
        "SOS": segment(0xDA, bytes([nc]) + b"".join(bytes([comp_ids[c], (comp_huff[c][0] << 4) | comp_huff[c][1]]) for c in range(nc)) +
                       b"\x00\x3f\x00"),
    }
    if layout is None:
        layout = list(pre_sof) + ["DQT", "SOF", "DHT", "DRI"] + list(pre_sos) + ["SOS"]
    assert layout[-1] == "SOS" and layout.count("SOF") == 1
    head = b"\xff\xd8" + b"".join(seg[x] if isinstance(x, str) else bytes(x) for x in layout)

    codes = [(_canonical(*huff[(0, comp_huff[c][0])]), _canonical(*huff[(1, comp_huff[c][1])])) for c in range(nc)]
    order = [(0, bx, by) for by in range(vs) for bx in range(hs)] + [(c, 0, 0) for c in range(1, nc)]
    bits, pred, block_off, rst_off = _Bits(), [0] * nc, [], []
    rst_fill, rst_number = rst_fill or {}, rst_number or {}
    ri = restart or 0
    for m in range(mx * my):
        if ri and m and m % ri == 0:
            k = m // ri - 1
            bits.pad(pad_ones)
            bits.out += b"\xff" * rst_fill.get(k, 0)
            rst_off.append(len(head) + len(bits.out))
            bits.out += bytes([0xFF, 0xD0 + (rst_number.get(k, k) & 7)])
            pred = [0] * nc
        for c, bx, by in order:
            fx, fy = (hs, vs) if c == 0 else (1, 1)
            block_off.append(len(head) + len(bits.out))
            pred[c] = _put_block(bits, coefs[c][(m // mx) * fy + by, (m % mx) * fx + bx], pred[c], *codes[c])
    bits.pad(pad_ones)
    r = Written()
    r.scan_off, r.scan_end = len(head), len(head) + len(bits.out)
    r.data = head + bytes(bits.out) + b"\xff" * eoi_fill + b"\xff\xd9" + bytes(trailer)
    r.block_off, r.rst_off, r.mcus, r.blocks_per_mcu = block_off, rst_off, mx * my, len(order)
    return r
