"""The cases of tests/golden/jpeg_decode.npz (tools/gen_jpeg_golden.py), shared by the CPU and the GPU tests of the JPEG decoder."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")


class Case:
    def __init__(self, z, i, off, poff):
        self.name = str(z["names"][i])
        self.data = z["data"][off[i]:off[i + 1]].tobytes()
        self.reason, self.status, self.w, self.h, self.ncomp, self.hs, self.vs, self.ri = (int(v) for v in z["meta"][i])
        self.sha = str(z["sha256"][i])
        n = int(z["pixels_len"][i])
        self.pixels = z["pixels"][poff[i]:poff[i] + n].reshape(self.h, self.w, 3) if n else None


def load_cases():
    z = np.load(GOLDEN)
    off = np.concatenate([[0], np.cumsum(z["data_len"])])
    poff = np.concatenate([[0], np.cumsum(z["pixels_len"])])
    return [Case(z, i, off, poff) for i in range(len(z["names"]))]


CASES = load_cases()
ACCEPTED = [c for c in CASES if c.reason == 0 and c.status == 0]
