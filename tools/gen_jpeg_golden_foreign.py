"""Writes tests/golden/jpeg_decode_foreign.npz: the second fixture file of the JPEG decoder, for what Pillow's own encoder at thumbnail
sizes (tests/golden/jpeg_decode.npz) never produces.  Same layout as that file (tools/gen_jpeg_golden.py), plus one CRC32 per band of
16 pixel rows for images above 64 x 64 (band_crc, band_len).  Needs Pillow; the tests that read the file do not.
`python tools/gen_jpeg_golden_foreign.py` from the repository root regenerates the committed file byte for byte.

  size_*    Pillow-encoded: the two photograph sizes, and strips that cover width (five trips of the colour kernel's x loop, odd and
            even last columns), height (18 trips of its y loop, an odd chroma height) and ten full groups of 8 blocks cheaply.
  win_*     written by tests/jpeg_writer.py against the entropy kernel's byte window (tests/jpeg_window.py: WIN, HALF, window_starts):
            groups whose bytes run past the window's end, stuffed FF 00 pairs and RSTn markers across the window's end and across a
            16-byte line, restart intervals against the group size.  Every property is asserted here from the writer's offsets.
  s_*       header and entropy-stream variants other encoders write, at most 64 x 64.

Every case must decode in Pillow; Pillow's pixels (or their SHA-256) are what is stored.  What the library must do with a case is
written down here by hand from the parser's documented scope (docs/design/ingest.md), never taken from the library: accepted, a
parser reason, or a decoder status."""
import hashlib
import io
import os
import sys
import warnings

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import jpeg_ref as R  # noqa: E402
import jpeg_writer as W  # noqa: E402
from gen_jpeg_golden import encode, segments  # noqa: E402
from jpeg_window import BAND, LINE, WIN, band_crcs, window_starts  # noqa: E402

COLOURSPACE, MARKER = 10, 4       # SCD_JPEG_COLOURSPACE (parser reason), JPEG_EMARKER (decoder status)

# A table with one code per length 1 .. 16: the 16-bit code 0xFFFE carries (run 0, size 7), so a coefficient of +-127 costs 23 bits,
# most of them ones.  With the one-code DC table (category 0 only) a block of 63 such coefficients is about 280 bytes after stuffing.
LONG_AC = ([1] * 16, [0x00, 0x01, 0x02, 0x03, 0x04, 0x11, 0x05, 0x12, 0x21, 0x06, 0x31, 0x41, 0xF0, 0x13, 0x22, 0x07])
DC0 = ([1] + [0] * 15, [0])
LONG_HUFF = {(0, 0): DC0, (1, 0): LONG_AC}
ONES = [1] * 64
Q_LUMA = [4 + (k * 7) % 23 for k in range(64)]
Q_CHROMA = [6 + (k * 5) % 31 for k in range(64)]


def long_blocks(rng, counts, size=7):
    """A row of gray blocks; block i has counts[i] coefficients (indices 1 ..) of magnitude 2^size - 1 .. with random signs, DC 0."""
    a = np.zeros((1, len(counts), 64), dtype=np.int64)
    for i, n in enumerate(counts):
        mag = (1 << size) - 1 if size == 7 else rng.integers(1 << (size - 1), 1 << size, n)
        a[0, i, 1:1 + n] = np.where(rng.random(n) < 0.6, 1, -1) * mag
    return a


def light(rng, shape, dc=30, nac=6, amp=5):
    """Blocks with a random DC level and nac small coefficients among the first 20."""
    a = np.zeros(shape + (64,), dtype=np.int64)
    a[..., 0] = rng.integers(-dc, dc + 1, shape)
    for idx in np.ndindex(*shape):
        k = rng.choice(np.arange(1, 21), nac, replace=False)
        a[idx][k] = rng.integers(-amp, amp + 1, nac)
    return a


def planes(rng, w, h, layout, **kw):
    """Coefficient arrays for write(): layout 'gray', '444', '422' or '420'."""
    hs, vs = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}[layout]
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    if layout == "gray":
        return [light(rng, (my, mx), **kw)], (1, 1)
    return [light(rng, (my * vs, mx * hs), **kw), light(rng, (my, mx), **kw), light(rng, (my, mx), **kw)], (hs, vs)


def shift(n):
    """Segments that move the scan by n bytes (n = 0, or 4 .. )."""
    return [] if n == 0 else [W.com(n)]


def pil(data):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    cases = []          # (name, data, reason, status, w, h, ncomp, hs, vs, restart_interval)
    notes = []

    def add(name, data, w, h, ncomp, hs, vs, ri=0, reason=0, status=0):
        assert name not in [c[0] for c in cases], name
        cases.append((name, bytes(data), reason, status, w, h, ncomp, hs, vs, ri))

    def add_written(name, wr, w, h, ncomp, hs, vs, ri=0, **kw):
        add(name, wr.data, w, h, ncomp, hs, vs, ri, **kw)

    # ------------------------------------------------------------------------------------------------------------ size cases
    geom = {0: (3, 1, 1), 1: (3, 2, 1), 2: (3, 2, 2), None: (1, 1, 1)}
    sname = {0: "444", 1: "422", 2: "420", None: "gray"}

    def size_case(w, h, sub, seed, **kw):
        tag = "_rst" if "restart_marker_blocks" in kw else ""
        add("size_%dx%d_%s%s" % (w, h, sname[sub], tag), encode(w, h, sub, seed, **kw), w, h, *geom[sub], ri=kw.get("restart_marker_blocks", 0))

    size_case(500, 375, 2, 3001, quality=40)
    size_case(375, 500, 1, 3002, quality=30, restart_marker_blocks=-(-375 // 16))           # one MCU row of 16 x 8 MCUs
    for w in (1024, 1025):
        size_case(w, 16, 2, 3003 + w, quality=50)
        size_case(w, 16, 1, 3005 + w, quality=50)
    size_case(257, 9, 0, 3010, quality=60)
    size_case(640, 8, None, 3011, quality=60)
    size_case(16, 1100, 2, 3012, quality=50)
    size_case(8, 1100, None, 3013, quality=50)
    rst = cases[1]
    dri = [s for s in segments(rst[1]) if s[0] == 0xDD]
    assert len(dri) == 1 and int.from_bytes(rst[1][dri[0][1] + 4:dri[0][1] + 6], "big") == 24

    # ------------------------------------------------------------------------------------------------------------ window cases
    def gray_long(counts, seed, com=0, ri=None, size=7):
        rng = np.random.default_rng(seed)
        return W.write(8 * len(counts), 8, [long_blocks(rng, counts, size)], quant={0: ONES}, huff=LONG_HUFF, restart=ri, pre_sof=shift(com))

    # dense: one group of 8 blocks whose bytes run past the window (lane 0 reads the rest from global memory)
    wr = gray_long([63] * 8, 1)
    start = wr.scan_off & ~(LINE - 1)
    span = wr.scan_end - start
    assert span > WIN + LINE and wr.mcus == 8
    notes.append("win_dense_8: one group, scan bytes %d .. %d, window from %d: %d bytes, %d past the window's end" %
                 (wr.scan_off, wr.scan_end, start, span, span - WIN))
    add_written("win_dense_8", wr, 64, 8, 1, 1, 1)

    # dense, three groups: a light first group, so that the second starts mid-window (no reload) and runs through the window's end, and the
    # third reloads.  Without restart markers the decoder's position at a boundary is the next block's first byte o or up to 4 bytes
    # further (bytes fetched ahead); every such position must give the same verdict.
    wr, com = None, 0
    for com in [0] + list(range(4, 20)):
        rng = np.random.default_rng(2)
        blocks = np.concatenate([long_blocks(rng, [63] * 8, 5), long_blocks(rng, [63] * 16, 7)], 1)
        wr = W.write(192, 8, [blocks], quant={0: ONES}, huff=LONG_HUFF, pre_sof=shift(com))
        if 1 <= wr.block_off[16] % LINE <= LINE - 5:
            break
    start0, o1, o2 = wr.scan_off & ~(LINE - 1), wr.block_off[8], wr.block_off[16]
    assert all(window_starts([wr.scan_off, s1])[1] == start0 for s1 in range(o1, o1 + 5)), "the second group must not reload"
    assert o2 - 1 >= start0 + WIN + LINE, "the second group must run past the window's end"
    start2 = {window_starts([wr.scan_off, o1, s2])[2] for s2 in range(o2, o2 + 5)}
    assert start2 == {o2 & ~(LINE - 1)} and wr.scan_end - (o2 & ~(LINE - 1)) > WIN + LINE
    notes.append("win_dense_24: groups start at %d, %d, %d; window [%d, %d) serves groups 1 and 2 (group 2 starts %d bytes into it and "
                 "reads to %d, %d past its end); group 3 reloads at %d (phase %d) and reads %d bytes, %d past the end" %
                 (wr.scan_off, o1, o2, start0, start0 + WIN, o1 - start0, o2, o2 - start0 - WIN, o2 & ~(LINE - 1), o2 % LINE,
                  wr.scan_end - (o2 & ~(LINE - 1)), wr.scan_end - (o2 & ~(LINE - 1)) - WIN))
    add_written("win_dense_24", wr, 192, 8, 1, 1, 1)

    # a stuffed FF 00 pair with its FF on the last byte of the window and its 00 on the first byte outside, for every phase of the
    # scan's first byte in its 16-byte line
    coms = {(W.write(8, 8, [long_blocks(np.random.default_rng(0), [1])], quant={0: ONES}, huff=LONG_HUFF, pre_sof=shift(c)).scan_off) % LINE: c
            for c in [0] + list(range(4, 20))}
    assert sorted(coms) == list(range(LINE))
    for phase in range(LINE):
        for seed in range(100, 400):
            wr = gray_long([63] * 8, seed, coms[phase])
            end = (wr.scan_off & ~(LINE - 1)) + WIN
            if end < wr.scan_end and wr.data[end - 1] == 0xFF and wr.data[end] == 0x00:
                break
        else:
            raise SystemExit("no seed puts a stuffed pair across the window's end at phase %d" % phase)
        assert wr.scan_off % LINE == phase and wr.data[end - 1:end + 1] == b"\xff\x00" and wr.scan_off < end - 1
        notes.append("win_ff00_end_p%02d: scan from %d (phase %d), FF at %d = window end - 1, 00 at %d (seed %d)" %
                     (phase, wr.scan_off, phase, end - 1, end, seed))
        add_written("win_ff00_end_p%02d" % phase, wr, 64, 8, 1, 1, 1)

    # the same pair across the first 16-byte line of a reloaded window: two groups of 8 dense blocks with a restart marker between them,
    # so the position at the boundary is exactly the marker's
    # (phase 13 and up cannot be: the marker takes two bytes and a block's first byte, a 0 bit and seven 1 bits, is never FF).  The block
    # behind the marker opens with 0 .. 7 coefficients of +-1 (3 bits each), which moves the bit phase of the dense ones behind them.
    def two_groups(seed, lead, c):
        rng = np.random.default_rng(seed)
        blocks = long_blocks(rng, [63] * 16)
        blocks[0, 8, 1:1 + lead] = np.sign(blocks[0, 8, 1:1 + lead])
        return W.write(128, 8, [blocks], quant={0: ONES}, huff=LONG_HUFF, restart=8, pre_sof=shift(c))

    for phase in range(13):
        found = None
        for seed, lead in ((s, l) for s in range(500, 600) for l in range(8)):
            wr = two_groups(seed, lead, 0)                         # the content is the seed's; the COM only shifts it
            if wr.data[wr.rst_off[0] + LINE - 1 - phase] != 0xFF:
                continue
            c = (phase - wr.rst_off[0]) % LINE
            c += LINE if 1 <= c <= 3 else 0
            wr = two_groups(seed, lead, c)
            s1 = wr.rst_off[0]
            st = window_starts([wr.scan_off, s1])
            if s1 % LINE == phase and st[1] == s1 & ~(LINE - 1) != st[0] and wr.data[st[1] + LINE - 1:st[1] + LINE + 1] == b"\xff\x00":
                found = (seed, c, s1, st[1])
                break
        assert found, phase
        seed, c, s1, st1 = found
        assert s1 + 2 <= st1 + LINE - 1 and wr.data[s1:s1 + 2] == b"\xff\xd0"
        notes.append("win_ff00_line_p%02d: reload at the RST0 at %d (phase %d), window from %d, FF at %d = its line's last byte, 00 at %d "
                     "(seed %d)" % (phase, s1, phase, st1, st1 + LINE - 1, st1 + LINE, seed))
        add_written("win_ff00_line_p%02d" % phase, wr, 128, 8, 1, 1, 1, ri=8)

    # RSTn markers: restart interval 1 on 64 MCUs, light and heavy groups in turn so that every other group runs through the end of a
    # window it did not load; over the four files a marker's first byte falls on every phase of a 16-byte line, and in the first a
    # marker has its FF inside the window and its Dn outside
    def rst_file(seed, c):
        rng = np.random.default_rng(seed)
        counts = [int(rng.integers(16, 24)) if (i // 8) % 2 == 0 else int(rng.integers(54, 64)) for i in range(64)]
        wr = gray_long(counts, seed + 1, c, ri=1)
        pos = [wr.scan_off] + [wr.rst_off[8 * g - 1] for g in range(1, 8)]
        starts = window_starts(pos)
        straddle = [(k, r) for k, r in enumerate(wr.rst_off) if r == starts[(k + 1) // 8] + WIN - 1]
        return wr, starts, straddle

    phases = set()
    for k, c in enumerate((0, 5, 10, 15)):
        for seed in range(4000 + 1000 * k, 5000 + 1000 * k):
            wr, starts, straddle = rst_file(seed, c)
            if straddle or k:
                break
        assert (straddle or k) and len(wr.rst_off) == 63 and wr.mcus == 64
        for j, r in enumerate(wr.rst_off):
            assert wr.data[r] == 0xFF and wr.data[r + 1] == 0xD0 + (j & 7)
        phases |= {r % LINE for r in wr.rst_off}
        crossing = [g for g in range(8) if (wr.rst_off[8 * g + 7] if g < 7 else wr.scan_end) > starts[g] + WIN]
        notes.append("win_rst_shift%02d: 63 markers (numbers wrap 7 times), phases %s, window starts %s, groups that read past their "
                     "window %s, markers across a window's end %s (seed %d)" %
                     (c, sorted({r % LINE for r in wr.rst_off}), sorted(set(starts)), crossing, straddle, seed))
        if k == 0:
            j, r = straddle[0]
            assert wr.data[r] == 0xFF and 0xD0 <= wr.data[r + 1] <= 0xD7 and r + 1 == starts[(j + 1) // 8] + WIN
        add_written("win_rst_shift%02d" % c, wr, 512, 8, 1, 1, 1, ri=1)
    assert phases == set(range(LINE)), phases
    notes.append("win_rst_*: phases hit over the set: %s" % sorted(phases))

    # the restart interval against the group: 8 gray MCUs, two 4:2:2 or 4:4:4 MCUs, one 4:2:0 MCU per group
    quant = {0: Q_LUMA, 1: Q_CHROMA}
    for lay, w, h, intervals in (("gray", 64, 24, (1, 2, 5, 8)), ("422", 64, 24, (1, 2, 5, 8)), ("444", 40, 24, (4,)), ("420", 64, 48, (4,))):
        for ri in intervals:
            rng = np.random.default_rng(600 + ri + len(cases))
            coefs, samp = planes(rng, w, h, lay)
            wr = W.write(w, h, coefs, sampling=samp, quant=quant if lay != "gray" else {0: Q_LUMA}, restart=ri, pre_sof=[W.jfif()],
                         **({} if lay != "gray" else dict(huff={(0, 0): W.DC_LUMA, (1, 0): W.AC_LUMA})))
            assert len(wr.rst_off) == (wr.mcus - 1) // ri >= 1
            add_written("win_ri%d_%s" % (ri, lay), wr, w, h, 1 if lay == "gray" else 3, *samp, ri=ri)

    # ------------------------------------------------------------------------------------------------------------ stream cases
    def stream(name, lay="420", w=40, h=24, seed=0, reason=0, status=0, ri=None, meta_ri=None, content=None, **kw):
        rng = np.random.default_rng(7000 + len(cases) + seed)
        coefs, samp = planes(rng, w, h, lay)
        if content is not None:
            coefs = content(coefs)
        if lay == "gray":
            kw.setdefault("quant", {0: Q_LUMA})
            kw.setdefault("huff", {(0, 0): W.DC_LUMA, (1, 0): W.AC_LUMA})
        else:
            kw.setdefault("quant", quant)
        if "layout" not in kw:
            kw.setdefault("pre_sof", [W.jfif()])
        wr = W.write(w, h, coefs, sampling=samp, restart=ri, **kw)
        add_written("s_" + name, wr, w, h, 1 if lay == "gray" else 3, *samp, ri=(ri or 0) if meta_ri is None else meta_ri, reason=reason,
                    status=status)
        return wr

    h23 = {(0, 2): W.DC_LUMA, (1, 2): W.AC_LUMA, (0, 3): W.DC_CHROMA, (1, 3): W.AC_CHROMA}
    stream("sof0_tables23", "422", quant={3: Q_LUMA, 2: Q_CHROMA}, comp_quant=[3, 2, 2], huff=h23, comp_huff=[(2, 2), (3, 3), (3, 3)],
           dht_merged=True)
    stream("sof1_tables23", "444", w=33, h=17, sof=0xC1, quant={2: Q_LUMA, 3: Q_CHROMA}, comp_quant=[2, 3, 3], huff=h23,
           comp_huff=[(2, 2), (3, 3), (3, 3)])
    stream("sof1_gray", "gray", w=21, h=13, sof=0xC1)
    stream("dqt16", "420", quant16=(0, 1))
    stream("dqt16_gray", "gray", w=17, h=9, quant16=(0,))
    stream("gray_f22", "gray", w=41, h=27, gray_factors=0x22)
    stream("gray_f41", "gray", w=50, h=19, gray_factors=0x41)
    stream("gray_f14", "gray", w=19, h=50, gray_factors=0x14)
    stream("nojfif_ids123", "420", pre_sof=[])
    # libjpeg guesses YCbCr for ids it does not know and RGB for 'R','G','B'; the parser takes three components only where YCbCr is certain
    stream("nojfif_ids012", "420", pre_sof=[], comp_ids=[0, 1, 2], reason=COLOURSPACE)
    stream("nojfif_idsRGB", "444", pre_sof=[], comp_ids=[ord("R"), ord("G"), ord("B")], reason=COLOURSPACE)
    stream("adobe0", "444", pre_sof=[W.adobe(0)], reason=COLOURSPACE)
    stream("adobe1", "420", pre_sof=[W.adobe(1)])
    stream("adobe1_ids012", "422", pre_sof=[W.adobe(1)], comp_ids=[0, 1, 2])
    stream("adobe2", "444", pre_sof=[W.adobe(2)], reason=COLOURSPACE)
    stream("jfif_adobe0", "420", pre_sof=[W.jfif(), W.adobe(0)])
    stream("adobe0_jfif", "444", pre_sof=[W.adobe(0), W.jfif()])
    stream("app0_not_jfif", "420", pre_sof=[W.segment(0xE0, b"JFXX\0\x10" + bytes(8))])
    stream("fill_header", "420", layout=[b"\xff", W.jfif(), b"\xff\xff", "DQT", b"\xff", "SOF", b"\xff\xff\xff", "DHT", b"\xff", "SOS"],
           eoi_fill=2)
    stream("fill_gray", "gray", w=24, h=16, layout=[b"\xff\xff", "DQT", "SOF", b"\xff", "DHT", b"\xff\xff", "SOS"], eoi_fill=1)
    stream("trailing", "422", trailer=b"\x00\x01\xff\xd8\xff\xc0 bytes behind EOI \xff\xd9\xff")
    stream("dri0", "420", ri=0)
    stream("dri_mcus", "420", w=48, h=32, ri=6, meta_ri=6)                    # exactly the MCU count: no marker is due
    stream("dri_65535", "gray", w=24, h=16, ri=65535)
    stream("dri_twice", "422", w=64, h=16, ri=2, pre_sos=[], layout=[W.jfif(), "DQT", W.dri(3), "SOF", "DHT", "DRI", "SOS"])
    stream("dri_then_0", "444", w=24, h=16, ri=0, layout=[W.jfif(), W.dri(1), "DQT", "SOF", "DHT", "DRI", "SOS"])
    other_q = [1 + (k * 11) % 50 for k in range(64)]
    other_ac = (W.AC_LUMA[0], W.AC_LUMA[1][:40] + W.AC_LUMA[1][40:][::-1])
    stream("redefined", "420", layout=[W.jfif(), W.dqt((0, other_q, False), (1, other_q, True)), W.dht((1, 0, other_ac), (0, 1, W.DC_LUMA)), "DQT",
                                       "SOF", "DHT", "SOS"])
    stream("redefined_gray", "gray", w=24, h=16, layout=[W.dqt((0, other_q, False)), W.dht((1, 0, other_ac)), "SOF", "DQT", "DHT", "SOS"])
    stream("tables_after_sof", "422", layout=[W.jfif(), "SOF", "DHT", "DQT", "SOS"])
    stream("unused_tables", "420", layout=[W.jfif(), "DQT", W.dqt((2, other_q, False)), "SOF", "DHT", W.dht((1, 2, other_ac), (0, 3, DC0)), "SOS"])
    stream("all_on_tables0", "444", quant={0: Q_LUMA}, comp_quant=[0, 0, 0], huff={(0, 0): W.DC_LUMA, (1, 0): W.AC_LUMA},
           comp_huff=[(0, 0)] * 3)
    stream("luma1_chroma0", "420", quant={1: Q_LUMA, 0: Q_CHROMA}, comp_quant=[1, 0, 0],
           huff={(0, 1): W.DC_LUMA, (1, 1): W.AC_LUMA, (0, 0): W.DC_CHROMA, (1, 0): W.AC_CHROMA}, comp_huff=[(1, 1), (0, 0), (0, 0)])
    stream("dc1_ac0", "gray", w=24, h=16, huff={(0, 1): W.DC_CHROMA, (1, 0): W.AC_LUMA}, comp_huff=[(1, 0)])

    # entropy-coded segment
    stream("pad_zeros", "444", w=40, h=24, ri=2, pad_ones=False)
    stream("pad_zeros_gray", "gray", w=40, h=16, ri=3, pad_ones=False)

    def last_only(coefs):            # 62 zeros (three ZRLs and a run of 14), then index 63; no EOB
        for c in coefs:
            c[..., 1:] = 0
            c[..., 63] = np.where(c[..., 0] % 2 == 0, 3, -2)
        return coefs

    def full(coefs):                 # every block ends on index 63 without an EOB
        for c in coefs:
            c[..., 63] = np.where(c[..., 0] % 2 == 0, 1, -1)
        return coefs

    stream("zrl3_idx63", "gray", w=24, h=16, content=last_only)
    stream("zrl3_idx63_420", "420", w=24, h=16, content=last_only)
    stream("idx63_no_eob", "422", w=40, h=16, content=full)

    def cat11(coefs):                # flat blocks whose DC level alternates -1023, +1000, ...: differences of 2023 (category 11)
        c = coefs[0]
        c[...] = 0
        flat = c.reshape(-1, 64)
        flat[:, 0] = np.where(np.arange(len(flat)) % 2 == 0, -1023, 1000)
        return coefs

    q1 = [1] + Q_LUMA[1:]
    stream("dc_cat11", "gray", w=32, h=16, quant={0: q1}, content=cat11)
    # 16-bit codes in use, and symbols no block uses: the long table again, in blocks that mix its short and long codes
    def mixed(coefs):
        c = coefs[0]
        c[...] = 0
        rng = np.random.default_rng(9)
        for blk in c.reshape(-1, 64):                     # runs of 0 only: the table has few (run, size) pairs
            blk[1:13] = rng.choice([1, -1, 3, -6, 12, -25, 60, -100, 127], 12)
        return coefs
    stream("huff16_unused", "gray", w=32, h=16, quant={0: ONES}, huff=LONG_HUFF, content=mixed)

    # inside the scope of the parser, outside what the entropy decoder follows: these go to Pillow with a status
    stream("rst_fill", "422", w=64, h=16, ri=1, rst_fill={1: 1}, status=MARKER)
    stream("rst_wrong_number", "gray", w=48, h=16, ri=2, rst_number={1: 3}, status=MARKER)

    # ------------------------------------------------------------------------------------------------------------ the file
    names, blobs, pix, sha, bands = [], [], [], [], []
    meta = np.zeros((len(cases), 8), dtype=np.int32)
    pix_len = np.zeros(len(cases), dtype=np.int64)
    band_len = np.zeros(len(cases), dtype=np.int64)
    for k, (name, data, reason, status, w, h, ncomp, hs, vs, ri) in enumerate(cases):
        names.append(name)
        blobs.append(np.frombuffer(data, dtype=np.uint8))
        meta[k] = (reason, status, w, h, ncomp, hs, vs, ri)
        rgb = pil(data)                                               # every case decodes in Pillow, the rejected ones included
        assert rgb.shape == (h, w, 3), name
        if reason == 0 and status == 0 and not name.startswith("size_"):
            try:                                                      # the range guard must stay quiet on what the writer made
                same = np.array_equal(R.decode(data), rgb)
            except R.Rejected as e:
                raise SystemExit("%s trips the range guard (%s)" % (name, e))
            if not same:
                print("NOTE: the restatement differs from Pillow on", name)
        sha.append(hashlib.sha256(rgb.tobytes()).hexdigest())
        if w <= 64 and h <= 64:
            pix.append(rgb.reshape(-1))
            pix_len[k] = rgb.size
        else:
            bands.append(band_crcs(rgb))
            band_len[k] = len(bands[-1])
            assert band_len[k] == -(-h // BAND)
    out = os.path.join(ROOT, "tests", "golden", "jpeg_decode_foreign.npz")
    np.savez(out, names=np.array(names), data=np.concatenate(blobs), data_len=np.array([len(b) for b in blobs], dtype=np.int64),
             meta=meta, pixels=np.concatenate(pix), pixels_len=pix_len, sha256=np.array(sha), band_crc=np.concatenate(bands),
             band_len=band_len)
    for n in notes:
        print(n)
    print(out, os.path.getsize(out), "bytes,", len(cases), "cases,", sum(len(b) for b in blobs), "bytes of JPEG")


if __name__ == "__main__":
    main()
