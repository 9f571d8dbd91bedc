"""CPU checks of the host side of scd_amd/csrc/f32mm.h against its restatement (tests/f32mm_plan.py): the four workspace sizes over a sweep
(they depend on R and RB, so they pin the plans the kernels are launched with), the coverage of the ranges, and the regime every named
case of probe_cases, gmm_cases, gmm_full_cases and pca_cases is named for."""
import numpy as np
import pytest

import f32mm_plan as fp
import gmm_cases as gc
import gmm_full_cases as fc
import pca_cases as pca
import probe_cases as pc

# the n of the sweep: the edges of the two plans, the production cache, either side of the column sums' cap, the limit, and every case's n
EDGES = [1, 1023, 1024, 1793, 126976, 131072, 131073, fp.N_MAX]
CASE_N = sorted({s[0] for menu in (pc.shapes(), gc.shapes(), fc.shapes()) for s in menu.values()} | {s[0] for s in pca.GRAM_SHAPES})
# (d, width) at which one range more or less moves the size: a range's partial is a whole number of 256-byte units there
PINNING = [(32, 32), (129, 129), (1024, 640)]
PINNING_FULL = [(8, 32), (33, 5 * 32), (64, 1000)]


def sweep(unit):
    """(n, d, width) of a unit: its case shapes, the edges and the case n's at the pinning widths, and its target-bound shape."""
    menu = {"probe": pc.shapes(), "gmm": gc.shapes(), "gmm_full": fc.shapes()}.get(unit)
    shapes = list(menu.values()) if menu else [(n, d, 1) for n, d in pca.GRAM_SHAPES] + list(pca.TRANSFORM_SHAPES)
    for n in EDGES + CASE_N:
        shapes += [(n, d, w) for d, w in (PINNING_FULL if unit == "gmm_full" else PINNING)]
    return shapes + [fp.TARGET_BOUND[unit][0]]


UNITS = {"probe": ("scd_probe_ws_bytes", fp.probe_ws_bytes, lambda n, d, w: fp.probe_plan(n, d, w)),
         "gmm": ("scd_gmm_ws_bytes", fp.gmm_ws_bytes, lambda n, d, w: fp.gmm_plan(n, d, w)),
         "gmm_full": ("scd_gmm_full_ws_bytes", fp.gmm_full_ws_bytes, lambda n, d, w: fp.gmm_full_plan(n, d, w)),
         "pca": ("scd_pca_ws_bytes", fp.pca_ws_bytes, lambda n, d, w: fp.pca_plan(n, d))}


@pytest.fixture(scope="module")
def L():
    from scd_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------- the workspace sizes
@pytest.mark.parametrize("unit", list(UNITS))
def test_workspace_sizes_are_the_restated_layouts(L, unit):
    sym, restated, plan = UNITS[unit]
    shapes = sweep(unit)
    assert {n for n, _, _ in shapes} >= set(EDGES) | {5121, 5153, 40000, 126976, 140001}
    for n, d, w in shapes:
        if unit == "probe" and w < 2:
            continue
        got = getattr(L, sym)(n, d, w)
        assert got == restated(n, d, w), "%s(%d, %d, %d) = %d, the restated layout has %d (plan %s)" % (sym, n, d, w, got, restated(n, d, w), plan(n, d, w))


def test_a_range_more_or_less_moves_the_size():
    """At the pinning widths the size is strictly increasing in R and in RB, so the equality above pins both: a partial of x >= 256 bytes
    gives align(R x) < R x + 256 <= (R + 1) x <= align((R + 1) x).  (At the narrow widths of the device cases, 140,001 x 5 x 3 for one,
    a range's partial is 120 bytes and two plans can share a size; the same n is therefore swept at these widths too.)"""
    for d, w in PINNING:
        assert w * d * 8 >= 256 and d * d * 8 >= 256            # probe, gmm: part [R, c, d]; pca: part [R, d, d]
        assert fp.pad(w, 32) * 8 >= 256 and fp.pad(d, 32) * 8 >= 256            # gbpart, nkpart [RB, cp]; colpart [RB, dp32]
    for d, k in PINNING_FULL:
        assert k * d * 8 >= 256 and fp.pad(k, 32) * 8 >= 256    # gmm_full: s1part [R, k, d] (and part [R, k, d, d]); nkpart [RB, kp]
    for x in (256, 120 * 3, 129 * 129 * 8):
        sizes = [fp.align(R * x) for R in range(1, 66)]
        assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert fp.align(31 * 120) == fp.align(30 * 120)             # the narrow width that hides a range


# ------------------------------------------------------------------------------------------------- the ranges cover the rows
@pytest.mark.parametrize("unit", list(UNITS))
def test_ranges_tile_the_rows(unit):
    _, _, plan = UNITS[unit]
    for n, d, w in sweep(unit):
        p = plan(n, d, w)
        assert 1 <= p["R"] <= fp.MAX_RANGES and 1 <= p["RB"] <= fp.CS_RANGES, (n, d, w, p)
        assert p["rows"] % fp.CHAIN == 0                        # every range but the last is a whole number of chains
        for count, rows, last in ((p["R"], p["rows"], p["last"]), (p["RB"], p["cs_rows"], p["cs_last"])):
            assert (count - 1) * rows < n <= count * rows and 1 <= last == n - (count - 1) * rows <= rows, (n, d, w, p)
        if n <= 200000:                                         # the ranges as the kernels cut them, one by one
            for count, rows in ((p["R"], p["rows"]), (p["RB"], p["cs_rows"])):
                b = fp.range_bounds(n, count, rows)
                assert b[0][0] == 0 and b[-1][1] == n and all(lo < hi for lo, hi in b)
                assert all(b[q][1] == b[q + 1][0] for q in range(count - 1))
        if p["R"] > 1:
            assert p["rows"] >= 4 * fp.CHAIN                    # at least four chains a range
        if n > fp.CS_ROWS * fp.CS_RANGES:
            assert p["RB"] >= fp.CS_RANGES - 1 and p["cs_rows"] == fp.cdiv(n, fp.CS_RANGES)
        elif n % fp.CS_ROWS == 0:
            assert p["cs_rows"] == fp.CS_ROWS


def test_target_blocks_bind_where_the_cap_of_32_does_not():
    for unit, (shape, R) in fp.TARGET_BOUND.items():
        p = UNITS[unit][2](*shape)
        target = 512 if unit == "gmm" else 1024
        assert fp.cdiv(target, p["tiles"]) < min(fp.MAX_RANGES, fp.cdiv(shape[0], fp.CHAIN) // 4), unit
        assert p["R"] == R, (unit, p)
    assert fp.gmm_full_plan(126976, 64, 1000)["tiles"] == 256 and fp.probe_plan(27649, 1024, 640)["tiles"] == 40
    assert fp.pca_plan(30465, 1024)["tiles"] == 36 and fp.gmm_plan(30465, 768, 257)["tiles"] == 18


# ------------------------------------------------------------------------------------------------- the regime of every named case
@pytest.mark.parametrize("name", list(fp.NT_CASES))
def test_forward_cases_land_in_their_regime(name):
    shape, (nt, phantom) = fp.NT_CASES[name]
    assert pc.shapes()[name] == gc.shapes()[name] == pca.NAMED_TRANSFORM[name] == shape and shape in pca.TRANSFORM_SHAPES
    assert fp.fwd_dispatch(shape[2]) == (nt, phantom)
    assert fp.phantom_columns(shape[2]) == (32 * phantom, fp.pad(shape[2], 32)) == pca.phantom_columns(shape[2])
    for v in pc.VARIANTS:
        assert pc.shape_case(name, v)["undecided_cap"] == 0.0
    assert fp.probe_plan(*shape)["R"] == 1                      # the forward regime alone: one range


def test_forward_dispatch_over_every_width():
    for w in range(1, 1025):
        nt, phantom = fp.fwd_dispatch(w)
        tiles = fp.cdiv(w, 32)
        assert nt in (1, 2, 4, 8) and 0 <= phantom == 4 * nt - tiles and (nt == 1 or 4 * (nt // 2) < tiles)
    assert [fp.fwd_dispatch(w)[0] for w in (128, 129, 256, 257, 512, 513, 992, 1024)] == [1, 2, 2, 4, 4, 8, 8, 8]
    assert fp.fwd_dispatch(992)[1] == 1 and fp.fwd_dispatch(160)[1] == 3 and fp.fwd_dispatch(1024)[1] == 0


@pytest.mark.parametrize("name", list(fp.RANGE_CASES))
def test_range_cases_land_in_their_regime(name):
    want = fp.RANGE_CASES[name]
    plans = {}
    if "wide" in want:
        assert pc.shapes()[name] == gc.shapes()[name] == want["wide"]
        plans["probe"], plans["gmm"] = fp.probe_plan(*want["wide"]), fp.gmm_plan(*want["wide"])
    else:
        assert name not in pc.shapes() and name not in gc.shapes()
    if "gram" in want:
        assert pca.NAMED_GRAM[name] == want["gram"] and want["gram"] in pca.GRAM_SHAPES
        plans["pca"] = fp.pca_plan(*want["gram"])
    assert fc.shapes()[name] == want["full"]
    plans["gmm_full"] = fp.gmm_full_plan(*want["full"])
    for unit, p in plans.items():
        assert (p["R"], p["rows"], p["last"]) == (want["R"], want["rows"], want["last"]), (unit, p)
        if "RB" in want:
            assert (p["RB"], p["cs_rows"]) == (want["RB"], want["cs_rows"]), (unit, p)
    tiles = fp.RANGE_TILES.get(name, {})
    for key, unit in (("wide", "probe"), ("wide", "gmm"), ("gram", "pca"), ("full", "gmm_full")):
        if key in tiles and unit in plans:
            assert plans[unit]["tiles"] == tiles[key], (unit, plans[unit])
    if "JT" in tiles:
        assert plans["gmm_full"]["JT"] == tiles["JT"]
    n = want["full"][0]
    assert fc.shape_case(name)["undecided_cap"] == fp.undecided_cap(n) == (1e-3 if n >= 5121 else 0.0)


def test_what_the_range_cases_are_named_for():
    R = fp.RANGE_CASES
    assert R["ranges_x_tiles"]["last"] == 1 and R["stage_plus_one"]["last"] == fp.STAGE + 1
    assert fp.probe_plan(*R["ranges_x_tiles"]["wide"])["ctiles"] == fp.probe_plan(*R["ranges_x_tiles"]["wide"])["dtiles"] == 2
    assert fp.pca_plan(*R["ranges_x_tiles"]["gram"])["dtiles"] == 3
    assert R["cap32"]["R"] == fp.MAX_RANGES and R["cap32"]["rows"] == 5 * fp.CHAIN      # ranges of five chains
    assert R["production_n"]["rows"] == 16 * fp.CHAIN and R["production_n"]["cs_rows"] == fp.CS_ROWS
    cap = R["colsum_cap"]
    assert cap["RB"] == fp.CS_RANGES and cap["cs_rows"] % fp.CS_GROUPS != 0 and cap["wide"][0] > fp.CS_ROWS * fp.CS_RANGES
    assert fp.gmm_full_plan(*R["jt2_chains"]["full"])["JT"] == 2 and fp.cdiv(R["jt2_chains"]["full"][0], fp.CHAIN) == 4
    # the cases of before: one tile wherever R > 1 outside gmm_full, R = 2 at the most
    assert fp.probe_plan(*pc.shapes()["two_ranges"])["R"] == 2 and fp.probe_plan(*pc.shapes()["two_ranges"])["tiles"] == 1
    assert fp.probe_plan(*pc.shapes()["four_chains"])["R"] == 1 and fp.probe_plan(*pc.shapes()["four_chains"])["tiles"] == 3


def test_large_cases_run_in_three_variants_and_carry_the_cap():
    """The menus alone (the host test of each unit asserts the cap of every generated case against its restatement)."""
    for mod, menu in ((pc, pc.shapes()), (gc, gc.shapes()), (fc, fc.shapes())):
        for name, (n, _, _) in menu.items():
            got = pc.variants_of(name) if mod is pc else gc.variants_of(name, menu)
            want = (pc.LARGE_VARIANTS if mod is pc else gc.LARGE_VARIANTS) if n >= fp.LARGE_N else mod.VARIANTS
            assert got == want, (name, got)
    assert pc.LARGE_VARIANTS == ("base", "weights") and gc.LARGE_VARIANTS == ("unlabelled", "weights", "hard")
    assert np.isclose(fp.UNDECIDED_CAP, 1e-3) and fp.undecided_cap(5120) == 0.0 and fp.undecided_cap(5121) == fp.UNDECIDED_CAP
