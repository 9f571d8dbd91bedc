"""Writes tests/golden/jpeg_decode.npz: JPEG byte strings with Pillow's Image.open(f).convert('RGB') pixels (or, above 64x64, the
SHA-256 of those bytes), and the reject cases of the device decoder with the reason / status each must get.  Needs Pillow; the tests
that read the file do not.  `python tools/gen_jpeg_golden.py` from the repository root.  The file is an uncompressed .npz, so
tests/sanitize_jpeg.cpp reads it without a zip library.

Accepted cases: 50x37, 33x17, 16x16, 7x5, 5x40, 41x63 (odd sizes, partial MCUs, chroma width 3) in 4:4:4, 4:2:2, 4:2:0 and grayscale,
two of the five encoder settings each in rotation so that every (sampling, setting) pair occurs: quality 3 (range-limit wrap), 30 with
optimised tables, 75 with restart markers every 3 MCUs, 90, 100.  Then a 250x187 4:2:0 file at quality 90 and one with EXIF, ICC and
comment segments before the frame.
Restart files (quality 75) for 7x5 and 5x40 in every sampling.
Reject cases: progressive, CMYK, a 4-pixel-wide 4:2:0 file, two files whose DHT is over-subscribed at length 1 (parser); a file cut inside its scan, one with a scan byte replaced so
that the entropy decoder meets an undefined code or an index past 63, one whose DQT holds 16-bit entries of 65,535, and one with a
scan byte replaced so that an IDCT output leaves [-512, 511] while the coefficients stay small (device status).  The last one is kept
with Pillow's pixels: it is the file on which libjpeg's range-limit wrap and a clamp differ, and the installed Pillow shows the clamp
(libjpeg-turbo's SIMD IDCT saturates), which is why the decoder hands such a file to Pillow."""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(50, 37), (33, 17), (16, 16), (7, 5), (5, 40), (41, 63)]
SAMPLINGS = [("444", 0), ("422", 1), ("420", 2), ("gray", None)]
SETTINGS = [("q3", dict(quality=3)), ("q30opt", dict(quality=30, optimize=True)), ("q75rst", dict(quality=75, restart_marker_blocks=3)),
            ("q90", dict(quality=90)), ("q100", dict(quality=100))]


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * (3 + c) + yy * (5 - c)) % 256 for c in range(3)], -1) + rng.integers(-40, 41, (h, w, 3))
    return Image.fromarray(np.clip(base, 0, 255).astype(np.uint8), "RGB")


def encode(w, h, sub, seed, **kw):
    im = picture(w, h, seed)
    b = io.BytesIO()
    if sub is None:
        im.convert("L").save(b, "JPEG", **kw)
    else:
        im.save(b, "JPEG", subsampling=sub, **kw)
    return b.getvalue()


def segments(data):
    """[(marker, start, end)] of the segments before the scan; end of the last = start of the scan's bytes."""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        ln = (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + ln))
        p += 2 + ln
        if m == 0xDA:
            return out


def with_dqt_65535(data):
    out = bytearray(data[:2])
    for m, a, b in segments(data):
        if m != 0xDB:
            out += data[a:b]
            continue
        ids, o = [], a + 4
        while o < b:
            ids.append(data[o] & 15)
            o += 1 + (128 if data[o] >> 4 else 64)
        body = b"".join(bytes([0x10 | t]) + b"\xff" * 128 for t in ids)
        out += b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
    return bytes(out) + data[segments(data)[-1][2]:]


def with_bad_scan_byte(data):
    """The first single-byte replacement inside the scan after which the CPU decoder reports an undefined code or an index past 63."""
    from scd_amd import jpeg
    start = segments(data)[-1][2]
    for pos in range(start + 2, len(data) - 2):
        for v in (0xFE, 0xFD, 0xFB, 0xF7, 0x7F):
            if data[pos] in (0xFF, v) or data[pos - 1] == 0xFF:
                continue
            cand = data[:pos] + bytes([v]) + data[pos + 1:]
            try:
                jpeg.decode_jpeg_host(cand)
            except jpeg.JpegDecodeError as e:
                if e.status in (1, 2):
                    return cand, e.status
    raise SystemExit("no single-byte replacement gives an undefined code or an index past 63")


def with_sample_out_of_range(data):
    """The first single-byte replacement inside the scan after which the library reports the range guard, Pillow still decodes the
    file, and the restatement without the guard gives other pixels with the range-limit wrap than with a clamp."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_ref as R
    from scd_amd import jpeg
    start = segments(data)[-1][2]
    for pos in range(start + 2, len(data) - 2):
        for v in (0xE2, 0xD9, 0x1F, 0xF1):
            if data[pos] in (0xFF, v) or data[pos - 1] == 0xFF:
                continue
            cand = data[:pos] + bytes([v]) + data[pos + 1:]
            try:
                jpeg.decode_jpeg_host(cand)
                continue
            except jpeg.JpegDecodeError as e:
                if e.status != 5:
                    continue
            try:
                pil = np.asarray(Image.open(io.BytesIO(cand)).convert("RGB"))
                wrap, clamp = R.decode(cand, guard=False), R.decode(cand, plant="clamp_range", guard=False)
            except Exception:
                continue
            if not np.array_equal(wrap, clamp) and np.array_equal(clamp, pil):
                return cand
    raise SystemExit("no single-byte replacement separates the wrap from the clamp")


def main():
    cases = []          # (name, data, reason, status, w, h, ncomp, hs, vs, restart_interval)

    def add(name, data, reason, status, w, h, ncomp, hs, vs, ri=0):
        cases.append((name, data, reason, status, w, h, ncomp, hs, vs, ri))

    geom = {0: (3, 1, 1), 1: (3, 2, 1), 2: (3, 2, 2), None: (1, 1, 1)}
    i = 0
    for w, h in SIZES:
        for sname, sub in SAMPLINGS:
            for qi in (i % 5, (i + 2) % 5):
                qname, kw = SETTINGS[qi]
                add("%dx%d_%s_%s" % (w, h, sname, qname), encode(w, h, sub, 1000 + i, **kw), 0, 0, w, h, *geom[sub],
                    ri=3 if "restart_marker_blocks" in kw else 0)
            i += 1
    # restart intervals over partial MCUs at the two smallest shapes, in every sampling (where the rotation above left them out)
    for w, h in ((7, 5), (5, 40)):
        for sname, sub in SAMPLINGS:
            name = "%dx%d_%s_q75rst" % (w, h, sname)
            if name not in [c[0] for c in cases]:
                add(name, encode(w, h, sub, 2000 + w, quality=75, restart_marker_blocks=3), 0, 0, w, h, *geom[sub], ri=3)
    add("250x187_420_q90", encode(250, 187, 2, 77, quality=90), 0, 0, 250, 187, 3, 2, 2)
    exif = Image.Exif()
    exif[0x010E] = "a description"
    exif[0x0112] = 6                     # orientation: ignored by pil_loader and by this decoder
    b = io.BytesIO()
    picture(40, 30, 5).save(b, "JPEG", quality=85, subsampling=2, exif=exif.tobytes(), icc_profile=bytes(range(256)) * 3,
                            comment=b"a comment segment")
    add("40x30_420_exif_icc_com", b.getvalue(), 0, 0, 40, 30, 3, 2, 2)
    # rejected by the parser
    add("rej_progressive", encode(33, 17, 2, 6, quality=80, progressive=True), 4, 0, 33, 17, 3, 2, 2)
    b = io.BytesIO()
    picture(24, 20, 7).convert("CMYK").save(b, "JPEG", quality=80)
    add("rej_cmyk", b.getvalue(), 8, 0, 24, 20, 4, 0, 0)
    # a DHT that gives length 1 more codes than it can hold: 3 (the look-up fill would pass its 256 entries) and 255 (far past the table)
    for tag, n1 in (("small", 3), ("large", 255)):
        body = bytes([0x00, n1] + [0] * 15) + bytes(range(n1))
        add("rej_dht_oversubscribed_" + tag, b"\xff\xd8\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body + b"\xff\xd9", 13, 0, 0, 0, 0, 0, 0)
    add("rej_4wide_420", encode(4, 16, 2, 8, quality=80), 14, 0, 4, 16, 3, 2, 2)
    # accepted by the parser, rejected by the decoder
    good = encode(50, 37, 2, 9, quality=80)
    start = segments(good)[-1][2]
    add("rej_cut_scan", good[:start + (len(good) - start) // 2], 0, 3, 50, 37, 3, 2, 2)
    bad, st = with_bad_scan_byte(good)
    add("rej_bad_code", bad, 0, st, 50, 37, 3, 2, 2)
    add("rej_range_guard", with_dqt_65535(good), 0, 5, 50, 37, 3, 2, 2)
    add("rej_sample_range", with_sample_out_of_range(encode(41, 63, 1, 1021, quality=90)), 0, 5, 41, 63, 3, 2, 1)

    names, blobs, pix, sha = [], [], [], []
    meta = np.zeros((len(cases), 8), dtype=np.int32)
    pix_len = np.zeros(len(cases), dtype=np.int64)
    for k, (name, data, reason, status, w, h, ncomp, hs, vs, ri) in enumerate(cases):
        names.append(name)
        blobs.append(np.frombuffer(data, dtype=np.uint8))
        meta[k] = (reason, status, w, h, ncomp, hs, vs, ri)
        digest = ""
        if reason == 0 and (status == 0 or name == "rej_sample_range"):
            rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            assert rgb.shape == (h, w, 3)
            digest = hashlib.sha256(rgb.tobytes()).hexdigest()
            if w <= 64 and h <= 64:
                pix.append(rgb.reshape(-1))
                pix_len[k] = rgb.size
        sha.append(digest)
    out = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
    np.savez(out, names=np.array(names), data=np.concatenate(blobs), data_len=np.array([len(b) for b in blobs], dtype=np.int64),
             meta=meta, pixels=np.concatenate(pix), pixels_len=pix_len, sha256=np.array(sha))
    print(out, os.path.getsize(out), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
