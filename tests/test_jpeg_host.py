"""The JPEG parser and the CPU decoder (scd_amd/jpeg.py, scd_amd/csrc/jpeg.h / jpeg.hip; docs/design/ingest.md, "Device JPEG decode")
against Pillow's pixels: tests/golden/jpeg_decode.npz (tools/gen_jpeg_golden.py) and, where Pillow is installed, freshly encoded files.
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
from jpeg_cases import ACCEPTED, CASES, GOLDEN, ROOT  # noqa: E402


def check_pixels(case, got):
    assert got.dtype == np.uint8 and got.shape == (case.h, case.w, 3), case.name
    if case.pixels is not None:
        assert np.array_equal(got, case.pixels), case.name
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == case.sha, case.name


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


def test_parser_info_and_reason_codes():
    from scd_amd import jpeg
    for c in CASES:
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
    for c in ACCEPTED:
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
    for c in ACCEPTED:
        ref = R.decode(c.data)
        check_pixels(c, ref)
        assert np.array_equal(ref, jpeg.decode_jpeg_host(c.data)), c.name


@pytest.mark.parametrize("plant", [p for p in R.PLANTS if p != "clamp_range"])
def test_planted_mistake_changes_a_fixture_pixel(plant):
    """One rule of the restatement broken at a time (replication for fancy upsampling, the rounding terms swapped, the neighbour chroma
    row taken from the padding, the last column taken from the padded width, restarts that keep the DC predictors): every one must
    change a pixel of an accepted fixture, or the fixtures do not pin that rule."""
    hits = [c.name for c in ACCEPTED if c.w <= 64 and not np.array_equal(R.decode(c.data, plant=plant, guard=False), c.pixels)]
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
    over every fixture and 1,000 seeded corruptions, as a stand-alone program."""
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
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failures" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
