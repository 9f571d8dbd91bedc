"""The cases of tests/golden/jpeg_decode.npz (tools/gen_jpeg_golden.py: files Pillow's encoder wrote) and of
tests/golden/jpeg_decode_foreign.npz (tools/gen_jpeg_golden_foreign.py: photograph sizes, scans laid against the kernel's byte window,
headers and streams other encoders write), shared by the CPU and the GPU tests of the JPEG decoder."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_window import BAND, HALF, LINE, WIN, band_crcs, window_starts  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
GOLDEN_FOREIGN = os.path.join(ROOT, "tests", "golden", "jpeg_decode_foreign.npz")


class Case:
    def __init__(self, z, i, off, poff, boff):
        self.name = str(z["names"][i])
        self.data = z["data"][off[i]:off[i + 1]].tobytes()
        self.reason, self.status, self.w, self.h, self.ncomp, self.hs, self.vs, self.ri = (int(v) for v in z["meta"][i])
        self.sha = str(z["sha256"][i])
        n = int(z["pixels_len"][i])
        self.pixels = z["pixels"][poff[i]:poff[i] + n].reshape(self.h, self.w, 3) if n else None
        self.bands = z["band_crc"][boff[i]:boff[i + 1]] if boff is not None else np.zeros(0, dtype=np.uint32)


def load_cases(path=GOLDEN):
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["data_len"])])
    poff = np.concatenate([[0], np.cumsum(z["pixels_len"])])
    boff = np.concatenate([[0], np.cumsum(z["band_len"])]) if "band_len" in z.files else None
    return [Case(z, i, off, poff, boff) for i in range(len(z["names"]))]


def first_bad_band(case, got):
    """For a failure message: the first band of 16 pixel rows of `got` whose CRC32 is not the recorded one (None: no bands recorded,
    or all equal)."""
    if not len(case.bands) or got.shape != (case.h, case.w, 3):
        return None
    bad = np.nonzero(band_crcs(got) != case.bands)[0]
    return None if not len(bad) else "rows %d .. %d" % (BAND * int(bad[0]), min(BAND * int(bad[0]) + BAND, case.h) - 1)


CASES = load_cases()
ACCEPTED = [c for c in CASES if c.reason == 0 and c.status == 0]
FOREIGN = load_cases(GOLDEN_FOREIGN)
FOREIGN_ACCEPTED = [c for c in FOREIGN if c.reason == 0 and c.status == 0]
