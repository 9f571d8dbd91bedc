"""The JPEG parser and the CPU decoder (scd_amd/jpeg.py, scd_amd/csrc/jpeg.h / jpeg.hip; docs/design/ingest.md, "Device JPEG decode")
against Pillow's pixels: tests/golden/jpeg_decode.npz (tools/gen_jpeg_golden.py), tests/golden/jpeg_decode_foreign.npz
(tools/gen_jpeg_golden_foreign.py: photograph sizes, scans laid against the kernel's byte window, other encoders' headers and streams)
and, where Pillow is installed, freshly encoded files.
scd_jpeg_decode_host runs the functions the kernels run, so this is the device decoder's arithmetic on the CPU."""
import hashlib
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as R  # noqa: E402
import jpeg_writer as W  # noqa: E402
from jpeg_cases import (ACCEPTED, CASES, FOREIGN, FOREIGN_ACCEPTED, GOLDEN, GOLDEN_FOREIGN, HALF, LINE, ROOT, WIN, first_bad_band,  # noqa: E402
                        window_starts)


def check_pixels(case, got):
    assert got.dtype == np.uint8 and got.shape == (case.h, case.w, 3), case.name
    if case.pixels is not None:
        assert np.array_equal(got, case.pixels), case.name
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == case.sha, (case.name, first_bad_band(case, got))


def test_fixture_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 564 * 1024
    names = {c.name for c in CASES}
    for w, h in [(50, 37), (33, 17), (16, 16), (7, 5), (5, 40), (41, 63)]:
        for s in ("444", "422", "420", "gray"):
            assert sum(n.startswith("%dx%d_%s_" % (w, h, s)) for n in names) >= 2
    for w, h in [(7, 5), (5, 40)]:                                  # restart intervals over partial MCUs, in every sampling
        for s in ("444", "422", "420", "gray"):
            assert "%dx%d_%s_q75rst" % (w, h, s) in names
    for s in ("444", "422", "420", "gray"):
        for q in ("q3", "q30opt", "q75rst", "q90", "q100"):
            assert any(n.endswith("_%s_%s" % (s, q)) for n in names), (s, q)
    assert {"250x187_420_q90", "40x30_420_exif_icc_com", "rej_progressive", "rej_cmyk", "rej_4wide_420", "rej_cut_scan", "rej_bad_code",
            "rej_range_guard", "rej_sample_range", "rej_dht_oversubscribed_small", "rej_dht_oversubscribed_large"} <= names
    for c in CASES:
        assert (c.pixels is not None) == (c.sha != "" and c.w <= 64 and c.h <= 64), c.name


FOREIGN_NAMES = (
    ["size_500x375_420", "size_375x500_422_rst", "size_1024x16_420", "size_1024x16_422", "size_1025x16_420", "size_1025x16_422", "size_257x9_444",
     "size_640x8_gray", "size_16x1100_420", "size_8x1100_gray", "win_dense_8", "win_dense_24"] +
    ["win_ff00_end_p%02d" % p for p in range(16)] + ["win_ff00_line_p%02d" % p for p in range(13)] +
    ["win_rst_shift%02d" % c for c in (0, 5, 10, 15)] + ["win_ri%d_%s" % (r, s) for s in ("gray", "422") for r in (1, 2, 5, 8)] +
    ["win_ri4_444", "win_ri4_420"] +
    ["s_" + n for n in ("sof0_tables23", "sof1_tables23", "sof1_gray", "dqt16", "dqt16_gray", "gray_f22", "gray_f41", "gray_f14", "nojfif_ids123",
                        "nojfif_ids012", "nojfif_idsRGB", "adobe0", "adobe1", "adobe1_ids012", "adobe2", "jfif_adobe0", "adobe0_jfif",
                        "app0_not_jfif", "fill_header", "fill_gray", "trailing", "dri0", "dri_mcus", "dri_65535", "dri_twice", "dri_then_0",
                        "redefined", "redefined_gray", "tables_after_sof", "unused_tables", "all_on_tables0", "luma1_chroma0", "dc1_ac0",
                        "pad_zeros", "pad_zeros_gray", "zrl3_idx63", "zrl3_idx63_420", "idx63_no_eob", "dc_cat11", "huff16_unused", "rst_fill",
                        "rst_wrong_number")])
FOREIGN_REJECTED = {"s_nojfif_ids012": ("reason", 10), "s_nojfif_idsRGB": ("reason", 10), "s_adobe0": ("reason", 10), "s_adobe2": ("reason", 10),
                    "s_rst_fill": ("status", 4), "s_rst_wrong_number": ("status", 4)}


def test_foreign_fixture_file_is_small_and_complete():
    """The second file: every case family of docs/design/ingest.md ("What the tests pin") by name, Pillow's pixels for every case
    (the rejected ones too: Pillow decodes them all), band checksums for the large images, and the same size limit as the first."""
    assert os.path.getsize(GOLDEN_FOREIGN) < 564 * 1024
    assert [c.name for c in FOREIGN] == FOREIGN_NAMES
    for c in FOREIGN:
        assert c.sha != "" and (c.pixels is not None) == (c.w <= 64 and c.h <= 64), c.name
        assert len(c.bands) == (0 if c.pixels is not None else -(-c.h // 16)), c.name
        want = FOREIGN_REJECTED.get(c.name, ("reason", 0))
        assert (c.reason, c.status) == ((want[1], 0) if want[0] == "reason" else (0, want[1])), c.name
        assert c.name.startswith("size_") or len(c.data) < 12 * 1024, c.name
    assert len(FOREIGN_ACCEPTED) == len(FOREIGN) - len(FOREIGN_REJECTED)


def test_foreign_reject_cases_carry_exactly_the_recorded_code():
    """Three components that are not YCbCr with certainty by libjpeg's default_decompress_parms rule are the parser's to refuse
    (colourspace), although libjpeg guesses YCbCr for two of the four; a fill byte before an RSTn inside the scan and an RSTn with the
    wrong number are the entropy decoder's (marker_in_scan).  Pillow decodes all six, and gets them."""
    from scd_amd import jpeg
    seen = {}
    for c in FOREIGN:
        try:
            jpeg.decode_jpeg_host(c.data)
        except jpeg.JpegUnsupported as e:
            seen[c.name] = ("reason", e.reason)
        except jpeg.JpegDecodeError as e:
            seen[c.name] = ("status", e.status)
    assert seen == FOREIGN_REJECTED


def _scan_of(data):
    """(first byte of the scan, offset of EOI) by a marker walk of the test's own: the window cases have neither fill bytes nor bytes
    behind EOI."""
    p = 2
    while data[p + 1] != 0xDA:
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    assert data[-2:] == b"\xff\xd9"
    return p + 2 + ((data[p + 2] << 8) | data[p + 3]), len(data) - 2


def test_window_cases_lie_where_their_names_say():
    """The window rule (jpeg_window.window_starts) on hand-made positions, and the committed window cases against it, from the files'
    own bytes: the generator asserts the same from the writer's offsets when it makes them."""
    assert window_starts([150]) == [144] and window_starts([150, 1168, 1169, 2300]) == [144, 144, 1168, 2288]
    assert window_starts([0, HALF, HALF + 1, 2 * HALF + 1, 2 * HALF + 2]) == [0, 0, HALF, 2 * HALF, 2 * HALF]       # '>' HALF, not '>='
    by_name = {c.name: c for c in FOREIGN}
    a, e = _scan_of(by_name["win_dense_8"].data)
    assert e - (a & ~(LINE - 1)) > WIN + LINE
    for p in range(16):
        d = by_name["win_ff00_end_p%02d" % p].data
        a, e = _scan_of(d)
        end = (a & ~(LINE - 1)) + WIN
        assert a % LINE == p and end < e and d[end - 1:end + 1] == b"\xff\x00", p
    for p in range(13):                                 # 13 .. 15 cannot be: the marker's two bytes, then a first byte that is never FF
        d = by_name["win_ff00_line_p%02d" % p].data
        a, e = _scan_of(d)
        s1 = d.index(b"\xff\xd0", a)                      # the only marker of the scan: 16 blocks, restart interval 8
        st = window_starts([a, s1])
        assert s1 % LINE == p and st[1] == s1 & ~(LINE - 1) and st[1] != st[0] and d[st[1] + LINE - 1:st[1] + LINE + 1] == b"\xff\x00", p
    phases, straddles = set(), 0
    for c in (0, 5, 10, 15):
        d = by_name["win_rst_shift%02d" % c].data
        a, e = _scan_of(d)
        rst = [k for k in range(a, e) if d[k] == 0xFF and 0xD0 <= d[k + 1] <= 0xD7]
        assert len(rst) == 63 and [d[k + 1] - 0xD0 for k in rst] == [k & 7 for k in range(63)]
        phases |= {k % LINE for k in rst}
        starts = window_starts([a] + [rst[8 * g - 1] for g in range(1, 8)])
        straddles += sum(r == starts[(k + 1) // 8] + WIN - 1 for k, r in enumerate(rst))
    assert phases == set(range(LINE)) and straddles >= 1


def test_writer_round_trip_and_offsets():
    """tests/jpeg_writer.py against the restatement's reader: the coefficients that went in come out dequantised, block by block, and
    the offsets it reports are those of the blocks' first bytes and of the RSTn markers."""
    rng = np.random.default_rng(5)
    quant = {0: [3 + k % 7 for k in range(64)], 1: [2 + k % 5 for k in range(64)]}
    for (hs, vs), ri in (((1, 1), None), ((2, 1), 2), ((2, 2), 1)):
        w, h = 37, 21
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        coefs = [rng.integers(-9, 10, s + (64,)) * (rng.random(s + (64,)) < 0.3) for s in ((my * vs, mx * hs), (my, mx), (my, mx))]
        coefs[0][0, 0, 1:] = 0
        coefs[0][0, 0, 63] = 5                                      # three ZRLs, a run of 14, no EOB
        wr = W.write(w, h, coefs, sampling=(hs, vs), quant=quant, restart=ri, pre_sof=[W.jfif()])
        q, huff, ri2, sof, sel, pos, jfif, adobe = R._header(wr.data)
        assert pos == wr.scan_off and ri2 == (ri or 0) and jfif and adobe is None and (sof["w"], sof["h"]) == (w, h)
        blocks = []
        R._scan(wr.data, pos, q, huff, ri2, sof["comps"], sel, hs, vs, mx, mx * my, None, blocks)
        assert len(blocks) == len(wr.block_off) == mx * my * (hs * vs + 2)
        for c, bx, by, coef in blocks:
            want = np.zeros(64, dtype=np.int64)
            want[R.ZIGZAG] = coefs[c][by, bx] * np.array(quant[min(c, 1)])
            assert np.array_equal(np.array(coef), want), (hs, vs, c, bx, by)
        assert wr.block_off[0] == wr.scan_off and all(a <= b for a, b in zip(wr.block_off, wr.block_off[1:]))
        assert wr.data[wr.scan_end:wr.scan_end + 2] == b"\xff\xd9" and len(wr.rst_off) == ((mx * my - 1) // ri if ri else 0)
        for k, o in enumerate(wr.rst_off):
            assert wr.data[o] == 0xFF and wr.data[o + 1] == 0xD0 + (k & 7)
            assert o + 2 in wr.block_off                            # the next block starts behind the marker


def test_parser_info_and_reason_codes():
    from scd_amd import jpeg
    for c in CASES + FOREIGN:
        i = jpeg.jpeg_info(c.data)
        assert i["reason"] == c.reason, (c.name, i)
        if c.reason != 0:
            continue
        assert (i["w"], i["h"], i["ncomp"], i["hs"], i["vs"], i["restart_interval"]) == (c.w, c.h, c.ncomp, c.hs, c.vs, c.ri), (c.name, i)
        sos = i["scan_off"] - (8 + 2 * c.ncomp)
        assert c.data[sos:sos + 2] == b"\xff\xda" and i["scan_off"] <= i["scan_end"] <= len(c.data), c.name
        assert i["has_eoi"] == (c.name != "rej_cut_scan"), c.name
        if i["has_eoi"]:
            assert c.data[i["scan_end"]:i["scan_end"] + 2] == b"\xff\xd9", c.name
        info, rst = jpeg.parse(c.data, restarts=True)
        mcus = -(-c.w // (8 * c.hs)) * -(-c.h // (8 * c.vs))
        if c.status == 0:
            assert len(rst) == i["n_restarts"] == ((mcus - 1) // c.ri if c.ri else 0), c.name
            for k, o in enumerate(rst):
                assert c.data[o] == 0xFF and c.data[o + 1] == 0xD0 + (k & 7), c.name
    assert jpeg.jpeg_info(b"")["reason_name"] == "not_jpeg" and jpeg.jpeg_info(b"\x89PNG\r\n\x1a\n" + b"\0" * 32)["reason_name"] == "not_jpeg"
    assert jpeg.jpeg_info(ACCEPTED[0].data[:100])["reason_name"] == "truncated_header"


def test_host_decode_equals_pillow_golden():
    from scd_amd import jpeg
    for c in ACCEPTED + FOREIGN_ACCEPTED:
        check_pixels(c, jpeg.decode_jpeg_host(c.data))


def test_host_decode_reject_cases():
    from scd_amd import jpeg
    seen = set()
    for c in CASES:
        if c.reason != 0:
            with pytest.raises(jpeg.JpegUnsupported) as e:
                jpeg.decode_jpeg_host(c.data)
            assert e.value.reason == c.reason, c.name
            seen.add(c.name)
        elif c.status != 0:
            with pytest.raises(jpeg.JpegDecodeError) as e:
                jpeg.decode_jpeg_host(c.data)
            assert e.value.status == c.status, c.name
            seen.add(c.name)
    assert seen == {"rej_progressive", "rej_cmyk", "rej_4wide_420", "rej_cut_scan", "rej_bad_code", "rej_range_guard", "rej_sample_range",
                    "rej_dht_oversubscribed_small", "rej_dht_oversubscribed_large"}
    bad = next(c for c in CASES if c.name == "rej_bad_code")
    assert bad.status in (1, 2)                                     # an undefined code or a coefficient index past 63


def test_oversubscribed_huffman_tables_are_refused_before_anything_is_written():
    """A DHT whose counts give a length more codes than it holds (3 or 255 codes of 1 bit, 129 of 7 bits, 2 of 1 bit, 2 after the
    first 254 codes of 8 bits) is a bad table, wherever it stands; the derived-table builder must say so before it fills its 256-entry look-up.  (The
    sanitizer program runs the two fixtures among these.)"""
    from scd_amd import jpeg
    for c in CASES:
        if c.name.startswith("rej_dht_oversubscribed"):
            assert jpeg.jpeg_info(c.data)["reason_name"] == "bad_table", c.name
    good = ACCEPTED[0].data
    p = good.index(b"\xff\xc4")
    for counts in ([3] + [0] * 15, [255] + [0] * 15, [0] * 6 + [129] + [0] * 9, [2, 1] + [0] * 14, [1, 1, 1, 1, 1, 1, 1, 2] + [0] * 8):
        body = bytes([0x00] + counts) + bytes(k % 12 for k in range(sum(counts)))
        seg = b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
        assert jpeg.jpeg_info(good[:p] + seg + good[p:])["reason_name"] == "bad_table", counts
    body = bytes([0x00] + [0] * 7 + [255] + [0] * 8) + bytes(k % 12 for k in range(255))       # 255 of the 256 codes of 8 bits: fine
    seg = b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
    assert jpeg.jpeg_info(good[:p] + seg + good[p:])["reason"] == 0


def test_frame_above_pillows_pixel_limit_is_pillows_to_judge(tmp_path):
    """A small file whose frame header claims 65,535 x 65,535 is inside the parser's scope, but above Pillow's MAX_IMAGE_PIXELS rule:
    read_for_device hands it to load_rgb, which raises what decode='pil' raises, and decode_jpeg_host allocates nothing for it."""
    pytest.importorskip("PIL.Image")
    from scd_amd import images, jpeg
    good = bytearray(next(c for c in ACCEPTED if c.name.startswith("50x37_420")).data)
    p = good.index(b"\xff\xc0")
    good[p + 5:p + 9] = b"\xff\xff\xff\xff"
    info = jpeg.parse(bytes(good))
    assert info["reason"] == 0 and (info["w"], info["h"]) == (65535, 65535) and jpeg.over_pillow_limit(info)
    with pytest.raises(jpeg.JpegUnsupported) as e:
        jpeg.decode_jpeg_host(bytes(good))
    assert e.value.reason == jpeg.TOO_LARGE
    path = tmp_path / "lying.jpg"
    path.write_bytes(bytes(good))
    errors = []
    for fn in (images.load_rgb, images.read_for_device):
        with pytest.raises(OSError, match="lying.jpg") as e:
            fn(str(path))
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "DecompressionBomb" in errors[0]
    assert not jpeg.over_pillow_limit(jpeg.parse(ACCEPTED[0].data))


def _picture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * (3 + c) + yy * (5 - c)) % 256 for c in range(3)], -1) + rng.integers(-60, 61, (h, w, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


def test_host_decode_equals_installed_pillow_on_fresh_files():
    """20 further sizes x 4 samplings x 3 encoder settings, encoded and decoded by the installed Pillow."""
    Image = pytest.importorskip("PIL.Image")
    from scd_amd import jpeg
    rng = np.random.default_rng(12)
    sizes = [(1, 1), (8, 8), (9, 1), (1, 17), (6, 3), (17, 2), (5, 2), (24, 24), (15, 31), (64, 48)]
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(5, 120, 10), rng.integers(1, 120, 10))]
    settings = [dict(quality=3), dict(quality=60, optimize=True, restart_marker_blocks=2), dict(quality=97)]
    n = 0
    for k, (w, h) in enumerate(sizes):
        for sub in (0, 1, 2, None):
            for kw in settings:
                im = Image.fromarray(_picture(w, h, 50 + k), "RGB")
                b = io.BytesIO()
                im.convert("L").save(b, "JPEG", **kw) if sub is None else im.save(b, "JPEG", subsampling=sub, **kw)
                data = b.getvalue()
                want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
                if sub in (1, 2) and (w + 1) // 2 <= 2:
                    assert jpeg.jpeg_info(data)["reason_name"] == "chroma_width", (w, h, sub)
                    continue
                assert np.array_equal(jpeg.decode_jpeg_host(data), want), (w, h, sub, kw)
                n += 1
    assert n >= 200


def test_restatement_equals_golden_and_library():
    from scd_amd import jpeg
    for c in ACCEPTED + FOREIGN_ACCEPTED:
        ref = R.decode(c.data)
        check_pixels(c, ref)
        assert np.array_equal(ref, jpeg.decode_jpeg_host(c.data)), c.name


PILLOW_WRITTEN_PLANTS = ("replicate", "swap_rounding", "unclamped_row", "padded_last_col", "clamp_range", "restart_keeps_pred")


@pytest.mark.parametrize("plant", [p for p in R.PLANTS if p != "clamp_range"])
def test_planted_mistake_changes_a_fixture_pixel(plant):
    """One rule of the restatement broken at a time (replication for fancy upsampling, the rounding terms swapped, the neighbour chroma
    row taken from the padding, the last column taken from the padded width, restarts that keep the DC predictors): every one must
    change a pixel of an accepted fixture, or the fixtures do not pin that rule.  Those six must be caught by the files Pillow's encoder
    wrote alone.  The others are about what only other encoders write, and must be caught by the second file: an Adobe transform 0
    beside JFIF taken for RGB, MCU geometry taken from a one-component frame's sampling factors, the first of two definitions of a table
    or of the restart interval kept, a ZRL that advances 15, pad bits that must be ones, a table id taken & 1."""
    cases = ACCEPTED if plant in PILLOW_WRITTEN_PLANTS else FOREIGN_ACCEPTED
    hits = [c.name for c in cases if c.pixels is not None and not np.array_equal(R.decode(c.data, plant=plant, guard=False), c.pixels)]
    assert hits, plant


def test_planted_clamp_for_the_range_limit_wrap():
    """libjpeg's C IDCT indexes its range-limit table with the low 10 bits of the output (a wrap); a clamp differs from it only for
    outputs outside [-512, 511].  No accepted fixture has such an output, quality 3 included; on rej_sample_range, which has one, the
    planted clamp changes pixels - and it is the clamp that equals Pillow's pixels there (libjpeg-turbo's SIMD IDCT saturates).  So
    the two cannot be told apart on any file the decoder takes, and a file where they differ gets the range-guard status and goes to
    Pillow: the guard's third bound."""
    from scd_amd import jpeg
    c = next(c for c in CASES if c.name == "rej_sample_range")
    wrap, clamp = R.decode(c.data, guard=False), R.decode(c.data, plant="clamp_range", guard=False)
    assert int((wrap != clamp).sum()) >= 1
    assert np.array_equal(clamp, c.pixels)
    with pytest.raises(R.Rejected, match="row pass"):
        R.decode(c.data)
    with pytest.raises(jpeg.JpegDecodeError) as e:
        jpeg.decode_jpeg_host(c.data)
    assert e.value.status == 5
    for a in ACCEPTED:
        if a.w <= 64:
            assert np.array_equal(R.decode(a.data, plant="clamp_range"), a.pixels), a.name


def test_range_guard_bounds():
    """The guard's three bounds on single blocks: a coefficient of 4097, a column-pass output above 8192, a row-pass output outside
    [-512, 511] are rejected; the largest values inside them are not."""
    blk = np.zeros((8, 8), dtype=np.int64)
    blk[0, 0] = 2048                                                # column pass 4 x 2048 = 8192, row pass 256: inside all three
    assert (R.idct(blk) == 255).all()
    blk[0, 0] = 2049
    with pytest.raises(R.Rejected, match="column pass"):
        R.idct(blk)
    blk[0, 0] = 4097
    with pytest.raises(R.Rejected, match="coefficient"):
        R.idct(blk)
    blk[0, 0], blk[0, 1] = 2048, 2048                               # first sample of each row: 256 + 355
    with pytest.raises(R.Rejected, match="row pass"):
        R.idct(blk)
    blk[0, 0], blk[0, 1] = -2048, -2048
    with pytest.raises(R.Rejected, match="row pass"):
        R.idct(blk)


def test_host_code_under_sanitizers(tmp_path):
    """tests/sanitize_jpeg.cpp: the parser, the table builder and the CPU decoder under AddressSanitizer + UndefinedBehaviorSanitizer
    over every fixture of both files and 1,000 seeded corruptions, as a stand-alone program."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        clang = shutil.which("clang++")
    assert clang, "no clang++ to build tests/sanitize_jpeg.cpp with"
    src = os.path.join(ROOT, "scd_amd", "csrc")
    exe = str(tmp_path / "sanitize_jpeg")
    cmd = [clang, "-x", "c++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", src,
           os.path.join(src, "jpeg.hip"), os.path.join(ROOT, "tests", "sanitize_jpeg.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    r = subprocess.run([exe, GOLDEN, GOLDEN_FOREIGN], capture_output=True, text=True, timeout=600)
    assert "%d fixtures" % (len(CASES) + len(FOREIGN)) in r.stdout, r.stdout
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
