"""Plain-Python restatement of the baseline JPEG decode rules the device decoder follows (scd_amd/csrc/jpeg.h; docs/design/ingest.md):
Huffman decode with restarts, dequantisation, the islow IDCT, fancy chroma upsampling, fixed-point YCbCr -> RGB.  Written from the
rules, not from the library's code, so that the two can be compared; and with switches that plant one mistake each, for the
sensitivity tests (tests/test_jpeg_host.py): a fixture set is only worth keeping if every planted mistake changes a pixel of it."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

PLANTS = ("replicate", "swap_rounding", "unclamped_row", "padded_last_col", "clamp_range", "restart_keeps_pred", "adobe_ignored",
          "gray_sampling_used", "first_table_wins", "first_dri_wins", "zrl_15", "pad_ones_required", "table_id_masked")
# Plants that change how the stream is read.  A reader that loses the stream under one of them (an undefined code, an index past 63, a
# missing marker) stops there and leaves the remaining blocks zero, as a decoder that conceals errors would: the mistake then shows
# as pixels, which is what the sensitivity test looks at.
_STREAM_PLANTS = ("gray_sampling_used", "first_table_wins", "first_dri_wins", "zrl_15", "pad_ones_required", "table_id_masked")


class Rejected(Exception):
    """The range guard tripped (the only rejection this restatement models)."""


def _header(d, plant=None):
    """Tables, restart interval, frame, the scan's table selectors, the scan's first byte, and what the APPn segments say about colour
    (jfif, adobe transform or None).  A later DQT, DHT or DRI replaces an earlier one; 0xFF fill bytes may precede any marker."""
    q, huff, ri, sof, p = {}, {}, None, None, 2
    jfif, adobe = False, None
    tid = (lambda t: t & 1) if plant == "table_id_masked" else (lambda t: t)
    keep_first = plant == "first_table_wins"
    while True:
        assert d[p] == 0xFF
        while d[p + 1] == 0xFF:
            p += 1
        m, ln = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        s = d[p + 4:p + 2 + ln]
        if m == 0xE0:
            jfif = jfif or (len(s) >= 14 and s[:5] == b"JFIF\0")
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe":
                adobe = s[11]
        elif m == 0xDB:
            o = 0
            while o < len(s):
                pq, tq = s[o] >> 4, s[o] & 15
                n = 128 if pq else 64
                t = s[o + 1:o + 1 + n]
                if not (keep_first and tid(tq) in q):
                    q[tid(tq)] = [(t[2 * k] << 8) | t[2 * k + 1] for k in range(64)] if pq else list(t)
                o += 1 + n
        elif m == 0xC4:
            o = 0
            while o < len(s):
                counts = s[o + 1:o + 17]
                total = sum(counts)
                syms = s[o + 17:o + 17 + total]
                table, code, k = {}, 0, 0
                for l in range(1, 17):
                    for _ in range(counts[l - 1]):
                        table[(l, code)] = syms[k]
                        code += 1
                        k += 1
                    code <<= 1
                if not (keep_first and (s[o] >> 4, tid(s[o] & 15)) in huff):
                    huff[(s[o] >> 4, tid(s[o] & 15))] = table
                o += 17 + total
        elif m == 0xDD:
            if not (plant == "first_dri_wins" and ri is not None):
                ri = (s[0] << 8) | s[1]
        elif m in (0xC0, 0xC1):
            sof = dict(h=(s[1] << 8) | s[2], w=(s[3] << 8) | s[4], comps=[(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, tid(s[8 + 3 * c]))
                                                                          for c in range(s[5])])
        elif m == 0xDA:
            sel = [(tid(s[2 + 2 * c] >> 4), tid(s[2 + 2 * c] & 15)) for c in range(s[0])]
            return q, huff, ri or 0, sof, sel, p + 2 + ln, jfif, adobe
        p += 2 + ln


class _Bits:
    def __init__(self, d, pos):
        self.d, self.pos, self.acc, self.n = d, pos, 0, 0

    def bit(self):
        if self.n == 0:
            c = self.d[self.pos]
            self.pos += 1
            if c == 0xFF:
                assert self.d[self.pos] == 0
                self.pos += 1
            self.acc, self.n = c, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            if (l, code) in table:
                return table[(l, code)]
        raise AssertionError("undefined code")

    def value(self, s):
        if s == 0:
            return 0
        r = self.bits(s)
        return r if r >= (1 << (s - 1)) else r - (1 << s) + 1

    def restart(self, n, pad_ones_required=False):
        assert not pad_ones_required or self.acc & ((1 << self.n) - 1) == (1 << self.n) - 1      # the unread bits: pad bits of either value
        self.n = 0
        assert self.d[self.pos] == 0xFF and self.d[self.pos + 1] == 0xD0 + (n & 7)
        self.pos += 2


def _pass(v, shift):
    """One IDCT pass along the last axis of an int64 array [..., 8]."""
    i = [v[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) * 8192, (i[0] - i[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    r = 1 << (shift - 1)
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([(o + r) >> shift for o in out], -1)


def idct(coef, clamp_range=False, guard=True):
    """coef int [..., 8, 8] (dequantised, natural order) -> uint8 [..., 8, 8]."""
    c = np.asarray(coef, dtype=np.int64)
    if guard and np.abs(c).max() > 4096:
        raise Rejected("coefficient")
    ws = np.swapaxes(_pass(np.swapaxes(c, -1, -2), 11), -1, -2)                      # down the columns
    if guard and np.abs(ws).max() > 8192:
        raise Rejected("column pass")
    x = _pass(ws, 18)
    if guard and (x.min() < -512 or x.max() > 511):
        raise Rejected("row pass")
    if clamp_range:
        return np.clip(x + 128, 0, 255).astype(np.uint8)
    v = x & 1023
    return np.where(v < 128, 128 + v, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def _upsample(p, hs, vs, w, h, plant):
    """Chroma plane p (whole MCUs) -> int [h, w]: h2v1 / h2v2 fancy upsampling, truncated to the image."""
    if hs == 1:
        return p[:h, :w].astype(np.int64)
    dw = p.shape[1] if plant == "padded_last_col" else (w + 1) // 2
    out = np.zeros((h, 2 * dw), dtype=np.int64)
    for y in range(h):
        if vs == 1:
            s, edge_mul, shift, r_even, r_odd = p[y].astype(np.int64), 1, 2, 1, 2
            e_even = e_odd = 0                                   # out[0] = in[0], out[last] = in[last]
            edge_shift = 0
        else:
            ch = p.shape[0] if plant == "unclamped_row" else (h + 1) // 2
            cy = y >> 1
            ny = min(max(cy + 1 if y & 1 else cy - 1, 0), ch - 1)
            s, edge_mul, shift, r_even, r_odd = 3 * p[cy].astype(np.int64) + p[ny], 4, 4, 8, 7
            e_even, e_odd, edge_shift = 8, 7, 4
        if plant == "swap_rounding":
            r_even, r_odd, e_even, e_odd = r_odd, r_even, e_odd, e_even
        if plant == "replicate":
            out[y, 0::2] = out[y, 1::2] = p[y if vs == 1 else y >> 1, :dw]
            continue
        for i in range(dw):
            out[y, 2 * i] = (edge_mul * s[0] + e_even) >> edge_shift if i == 0 else (3 * s[i] + s[i - 1] + r_even) >> shift
            out[y, 2 * i + 1] = (edge_mul * s[i] + e_odd) >> edge_shift if i == dw - 1 else (3 * s[i] + s[i + 1] + r_odd) >> shift
    return out[:, :w]


def _scan(d, pos, q, huff, ri, comps, sel, hs, vs, mx, n_mcu, plant, blocks):
    """The entropy-coded segment: appends (component, block column, block row, 64 dequantised coefficients in natural order)."""
    nc = len(comps)
    layout = [(0, bx, by) for by in range(vs) for bx in range(hs)] + [(c, 0, 0) for c in range(1, nc)]
    bits, pred = _Bits(d, pos), [0] * nc
    for m in range(n_mcu):
        if ri and m and m % ri == 0:
            bits.restart(m // ri - 1, plant == "pad_ones_required")
            if plant != "restart_keeps_pred":
                pred = [0] * nc
        for c, bx, by in layout:
            qt, dc, ac = q[comps[c][3]], huff[(0, sel[c][0])], huff[(1, sel[c][1])]
            coef = [0] * 64
            pred[c] += bits.value(bits.symbol(dc))
            coef[0] = pred[c] * qt[0]
            k = 1
            while k < 64:
                rs = bits.symbol(ac)
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    assert k < 64
                    coef[ZIGZAG[k]] = bits.value(s) * qt[k]
                    k += 1
                elif r == 15:
                    k += 15 if plant == "zrl_15" else 16
                else:
                    break
            fx, fy = (hs, vs) if c == 0 else (1, 1)
            blocks.append((c, (m % mx) * fx + bx, (m // mx) * fy + by, coef))


def decode(data, plant=None, guard=True):
    """JPEG bytes -> uint8 [h, w, 3] by the rules; plant: one of PLANTS (or None); guard: apply the range guard (Rejected)."""
    assert plant is None or plant in PLANTS
    d = bytes(data)
    q, huff, ri, sof, sel, pos, jfif, adobe = _header(d, plant)
    w, h, comps = sof["w"], sof["h"], sof["comps"]
    nc = len(comps)
    # a one-component scan is one block per MCU whatever the frame's sampling factors say
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 or plant == "gray_sampling_used" else (1, 1)
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    planes = [np.zeros((my * 8 * (vs if c == 0 else 1), mx * 8 * (hs if c == 0 else 1)), dtype=np.uint8) for c in range(nc)]
    blocks = []
    try:
        _scan(d, pos, q, huff, ri, comps, sel, hs, vs, mx, mx * my, plant, blocks)
    except (AssertionError, IndexError, KeyError):
        if plant not in _STREAM_PLANTS:
            raise
    if blocks:
        px = idct(np.array([b[3] for b in blocks]).reshape(-1, 8, 8), plant == "clamp_range", guard)
        for (c, bx, by, _), p8 in zip(blocks, px):
            planes[c][8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = p8
    if nc == 3:
        # libjpeg's default_decompress_parms: JFIF means YCbCr whatever Adobe says; else Adobe's transform; else the component ids
        ycc = jfif or adobe == 1 or (adobe is None and [c[0] for c in comps] == [1, 2, 3])
        if plant == "adobe_ignored":
            ycc = adobe != 0                  # the plant: an Adobe transform 0 means RGB although a JFIF segment stands beside it
        assert ycc or plant == "adobe_ignored", "outside the decoder's scope: not YCbCr with certainty"
    yy = planes[0][:h, :w].astype(np.int64)
    if nc == 1:
        return np.repeat(yy[:, :, None], 3, 2).astype(np.uint8)
    cb = _upsample(planes[1], hs, vs, w, h, plant) - 128
    cr = _upsample(planes[2], hs, vs, w, h, plant) - 128
    if not ycc:
        return np.stack([yy, cb + 128, cr + 128], -1).astype(np.uint8)
    rgb = np.stack([yy + ((91881 * cr + 32768) >> 16), yy + ((-22554 * cb - 46802 * cr + 32768) >> 16), yy + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)
