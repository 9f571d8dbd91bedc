"""The host side of scd_amd/csrc/f32mm.h restated in plain Python: the row-range plans of the A^T B kernels and of the column sums, the
forward kernels' dispatch on tiles per wave, and each unit's tile count and workspace layout (probe.hip, gmm.hip, gmm_full.hip, pca.hip).
tests/test_f32mm_plan_host.py holds the library to it through the four scd_*_ws_bytes, whose values depend on R and RB; the case modules
take the regime of every named case from here."""

CHAIN = 256                                     # F32MM_CHAIN: rows of a float32 accumulation chain
GT = 128                                        # F32MM_GT: the tile of A^T B
STAGE = 32                                      # F32MM_GK: rows per LDS stage
MAX_RANGES = 32                                 # the cap of f32mm_ranges
CS_ROWS = 2048                                  # F32MM_CS_ROWS
CS_RANGES = 64                                  # F32MM_CS_RANGES
CS_GROUPS = 8                                   # row groups of f32mm_colsum
GMMF_CG = 4                                     # components of a gmm_full moment block
N_MAX = (1 << 31) - 1


def cdiv(a, b):
    return -(-a // b)


def pad(v, to):
    return cdiv(v, to) * to


def align(x, a=256):
    return cdiv(x, a) * a


# ------------------------------------------------------------------------------------------------- the two range plans
def ranges(n, tiles, target_blocks):
    """f32mm_ranges: (R, rows_per_range).  At least four chains a range, at most 32 ranges and about target_blocks blocks, a whole
    number of chains per range."""
    chains = cdiv(n, CHAIN)
    r = max(1, min(chains // 4, MAX_RANGES, cdiv(target_blocks, tiles)))
    rows = cdiv(chains, r) * CHAIN
    return cdiv(n, rows), rows


def colsum_ranges(n):
    """f32mm_colsum_ranges: (RB, rows_per_range)."""
    r = min(cdiv(n, CS_ROWS), CS_RANGES)
    rows = cdiv(n, r)
    return cdiv(n, rows), rows


def range_bounds(n, count, rows):
    """[(lo, hi)] of the `count` ranges of `rows` rows over [0, n), as f32mm_range cuts them."""
    return [(q * rows, min((q + 1) * rows, n)) for q in range(count)]


# ------------------------------------------------------------------------------------------------- the forward dispatch
def fwd_dispatch(width):
    """f32mm_fwd_dispatch for an operand of `width` rows (classes, components, columns): (NT, phantom tiles).  The padded width / 32
    tiles go over four waves, NT = 1, 2, 4 or 8 tiles a wave; the 4 NT - tiles tiles past the padded width are phantom."""
    tiles = pad(width, 32) // 32
    per = cdiv(tiles, 4)
    nt = 1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8
    return nt, 4 * nt - tiles


def phantom_columns(width):
    """(columns a block computes beyond the padded width, the padded width)."""
    nt, _ = fwd_dispatch(width)
    wp = pad(width, 32)
    return 4 * nt * 32 - wp, wp


# ------------------------------------------------------------------------------------------------- the units' plans
def _plan(n, tiles, target):
    R, rows = ranges(n, tiles, target)
    RB, cs_rows = colsum_ranges(n)
    return dict(n=n, tiles=tiles, R=R, rows=rows, last=n - (R - 1) * rows, RB=RB, cs_rows=cs_rows, cs_last=n - (RB - 1) * cs_rows)


def probe_plan(n, d, c):
    """Gradient tiles: (class tiles of 128 over the padded classes) x (dim tiles), about 1024 blocks."""
    p = _plan(n, cdiv(pad(c, 32), GT) * cdiv(d, GT), 1024)
    p.update(ctiles=cdiv(pad(c, 32), GT), dtiles=cdiv(d, GT))
    return p


def gmm_plan(n, d, k):
    """The same tiles as the probe's; 512, about 1024 blocks over the two moments."""
    p = _plan(n, cdiv(pad(k, 32), GT) * cdiv(d, GT), 512)
    p.update(ctiles=cdiv(pad(k, 32), GT), dtiles=cdiv(d, GT))
    return p


def gmm_full_plan(n, d, k):
    """Moment blocks of four components; JT = the j-tiles of 32 of a component's matrix."""
    p = _plan(n, pad(k, 32) // GMMF_CG, 1024)
    p.update(JT=cdiv(d, 32))
    return p


def pca_plan(n, d):
    """Upper-triangle tiles of the Gram matrix."""
    dt = cdiv(d, GT)
    p = _plan(n, dt * (dt + 1) // 2, 1024)
    p.update(dtiles=dt)
    return p


# ------------------------------------------------------------------------------------------------- the workspaces, byte for byte
def probe_ws_bytes(n, d, c):
    p, cp, dp = probe_plan(n, d, c), pad(c, 32), pad(d, 8)
    return (align(cp * dp * 4) + align(n * cp * 4) + align(n * 4)           # Wp f32 [cp, dp], r f32 [n, cp], rowloss f32 [n]
            + align(p["R"] * c * d * 8)                                     # part f64 [R, c, d]
            + align(p["RB"] * cp * 8) + align(p["RB"] * 8))                 # gbpart f64 [RB, cp], losspart f64 [RB]


def gmm_ws_bytes(n, d, k):
    p, kp, dp = gmm_plan(n, d, k), pad(k, 32), pad(d, 8)
    return (align(kp * 2 * dp * 4) + align(n * kp * 4) + align(n * 8)       # BCp f32 [kp, 2 dp], r f32 [n, kp], rowll f64 [n]
            + align(2 * p["R"] * k * d * 8)                                 # part f64 [2, R, k, d]
            + align(p["RB"] * kp * 8) + align(p["RB"] * 8))                 # nkpart f64 [RB, kp], llpart f64 [RB]


def gmm_full_ws_bytes(n, d, k):
    p, kp, dp, jp = gmm_full_plan(n, d, k), pad(k, 32), pad(d, 8), pad(d, 32)
    return (align(k * jp * dp * 4) + align(k * dp * 4)                      # Utp f32 [k, jp, dp], mup f32 [k, dp]
            + align(n * kp * 4) + align(n * 8)                              # r f32 [n, kp], rowll f64 [n]
            + align(p["R"] * k * d * d * 8) + align(p["R"] * k * d * 8)     # part f64 [R, k, d, d], s1part f64 [R, k, d]
            + align(p["RB"] * kp * 8) + align(p["RB"] * 8))                 # nkpart f64 [RB, kp], llpart f64 [RB]


def pca_ws_bytes(n, d, m):
    p, mp, dp, dp32 = pca_plan(n, d), pad(m, 32), pad(d, 8), pad(d, 32)
    return (align(d * 4) + align(p["RB"] * dp32 * 8) + align(n * 4)         # zeros f32 [d], colpart f64 [RB, dp32], flags i32 [n]
            + align(p["R"] * d * d * 8) + align(mp * dp * 4))               # part f64 [R, d, d], Wp f32 [mp, dp]


# ------------------------------------------------------------------------------------------------- the named cases and their regimes
# name -> (n, d, width) of probe and gmm (pca: the transform's (n, d, m)); the forward regime each must hit: (NT, phantom tiles)
NT_CASES = {"nt2_phantom": ((103, 64, 129), (2, 3)), "nt2_exact": ((33, 40, 256), (2, 0)), "nt8_phantom": ((65, 24, 545), (8, 14))}

# name -> the shapes of probe / gmm (n, d, width), gmm_full (n, d, k), pca Gram (n, d), and the plan each must hit:
# R, the last range's rows; RB and the column sums' rows per range where the case is named for them
RANGE_CASES = {
    "ranges_x_tiles": dict(wide=(5121, 129, 129), full=(5121, 64, 9), gram=(5121, 257), R=5, rows=1280, last=1),
    "stage_plus_one": dict(wide=(5153, 129, 33), full=(5153, 33, 5), gram=(5153, 129), R=5, rows=1280, last=STAGE + 1),
    "jt2_chains": dict(full=(773, 33, 5), R=1, rows=1024, last=773),
    "cap32": dict(wide=(40000, 129, 33), full=(40000, 17, 9), gram=(40000, 33), R=32, rows=1280, last=320, RB=20, cs_rows=2000),
    "production_n": dict(wide=(126976, 40, 40), full=(126976, 8, 5), gram=(126976, 40), R=31, rows=4096, last=4096, RB=62, cs_rows=2048),
    "colsum_cap": dict(wide=(140001, 5, 3), full=(140001, 5, 3), gram=(140001, 5), R=31, rows=4608, last=1761, RB=64, cs_rows=2188),
}
# what else the table of the cases promises: the tiles the several ranges meet
RANGE_TILES = {"ranges_x_tiles": dict(wide=4, gram=6, full=8, JT=2), "jt2_chains": dict(full=8, JT=2)}

# the shapes at which about target_blocks blocks bind, not the 32 ranges: host arithmetic alone, so no device case
TARGET_BOUND = {"probe": ((27649, 1024, 640), 22), "pca": ((30465, 1024, 1), 24), "gmm": ((30465, 768, 257), 24),
                "gmm_full": ((126976, 64, 1000), 4)}

LARGE_N = 5121                                  # from here on a case carries an undecided_cap and runs in three variants
UNDECIDED_CAP = 1e-3                            # 0.1 % of the rows may have a top-two gap within 2 delta


def undecided_cap(n):
    return UNDECIDED_CAP if n >= LARGE_N else 0.0
