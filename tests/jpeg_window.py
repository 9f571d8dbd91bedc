"""What the window cases of tests/golden/jpeg_decode_foreign.npz are laid against, for the generator (tools/gen_jpeg_golden_foreign.py)
and the tests alike: the byte-window rule of jpeg_entropy_idct_kernel, and the band checksums of the large images."""
import zlib

import numpy as np

BAND = 16        # pixel rows per CRC band of an image above 64 x 64


def band_crcs(rgb):
    """CRC32 of every band of BAND pixel rows of a uint8 [h, w, 3] image."""
    rgb = np.ascontiguousarray(rgb)
    return np.array([zlib.crc32(rgb[y:y + BAND].tobytes()) for y in range(0, rgb.shape[0], BAND)], dtype=np.uint32)


# jpeg_entropy_idct_kernel reads the scan through a window of WIN bytes in LDS (scd_amd/csrc/jpeg.hip, JpegWinSrc).  The rule its
# comment states, restated here as estep_cases.path restates its dispatcher: at every group boundary (a group is 8 / blocks-per-MCU
# whole MCUs), with s the scan position there, the window is reloaded from s & ~15 when s is more than HALF past the window's start;
# a byte outside [start, start + WIN) is read from global memory.
WIN, HALF, LINE = 2048, 1024, 16


def window_starts(positions):
    """Scan positions at the group boundaries, in order -> the window start in force while each group is decoded."""
    start, out = -WIN, []
    for s in positions:
        if s - start > HALF:
            start = s & ~(LINE - 1)
        out.append(start)
    return out
