"""The shapes of tests/fold_scale_cases.py cross the grid caps of the step-3 folds.

The GPU tests that run those shapes cover the multi-unit loops (a workgroup's second and third
tile, a thread's second trip) only as long as the caps in the sources stay where they are.
This test reads the caps from the .hip / .h sources, compares them with the constants the
plan restatements of fold_scale_cases.py use, and asserts per case what its comment claims:
units per workgroup, workgroups that straddle two walkers, a shorter last workgroup, a
workgroup none of whose units is used.  A cap that moves fails here instead of silently
turning the coverage off.
"""
import os
import re

import pytest

import fold_scale_cases as fc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olpefit_amd",
                    "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def const(text, name):
    """The integer value of `constexpr <type> name = <expr>;` (products, shifts, ll / ull)."""
    m = re.search(r"constexpr\s+[\w ]+?\b%s\s*=\s*([^;]+);" % re.escape(name), text)
    assert m, name
    expr = re.sub(r"(\d)(?:ull|ll|u)\b", r"\1", m.group(1))
    assert re.fullmatch(r"[\d\s*<>()+-]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}))


def test_the_caps_are_the_sources():
    cov, acf, sel = source("olpe_cov.hip"), source("olpe_acf.hip"), source("olpe_select.h")
    assert const(cov, "kMaxSlots") == fc.COV_MAX_SLOTS
    assert const(cov, "kDefaultTile") == fc.COV_DEFAULT_TILE
    tiles = re.search(r"constexpr int kTiles\[\]\s*=\s*\{([^}]*)\}", cov).group(1)
    assert [int(t) for t in tiles.split(",")] == [64, 128, 256]
    assert "std::min<long long>(a.tiles, kMaxSlots)" in cov
    assert const(acf, "kMaxSlots") == fc.ACF_MAX_SLOTS
    assert (const(acf, "kSub"), const(acf, "kMaxTile"), const(acf, "kMaxGroup")) == \
        (fc.ACF_SUB, fc.ACF_MAX_TILE, fc.ACF_MAX_GROUP)
    assert const(acf, "kLdsBudget") == fc.ACF_LDS_BUDGET
    assert "std::min<long long>(a.units, kMaxSlots)" in acf
    assert const(sel, "kSelBlocks") * const(sel, "kSelThreads") == fc.SEL_THREADS
    for name in ("olpe_phot.hip", "olpe_astrom.hip"):
        text = source(name)
        assert const(text, "kThreads") == fc.REDUCE_THREADS, name
        assert const(text, "kThreads") * const(text, "kPer") == fc.REDUCE_CHUNK, name
        assert re.search(r"constexpr long long kChunk\s*=\s*kThreads \* kPer;", text), name
    # stage 2: phot's own kernel, and the shared one (olpe_reduce.h) astrom launches
    assert re.search(r"for \(int b = threadIdx\.x; b < nblk; b \+= kThreads\)",
                     source("olpe_phot.hip"))
    red, astrom = source("olpe_reduce.h"), source("olpe_astrom.hip")
    assert re.search(r"for \(int b = threadIdx\.x; b < nblk; b \+= T\)", red)
    assert "__launch_bounds__(T) void reduce_stage2_kernel(" in red
    assert "hipLaunchKernelGGL(reduce_stage2_kernel<kThreads>, dim3(nv), dim3(kThreads)," in astrom
    m = re.search(r"cgrid = \(unsigned\)std::min<long long>\(\(n \+ kThreads - 1\) / kThreads, "
                  r"(\d+)\)", astrom)
    assert m and int(m.group(1)) * const(astrom, "kThreads") == fc.CORRECT_THREADS
    corner = source("olpe_corner.hip")
    assert const(corner, "kStageSamples") == fc.CORNER_STAGE
    assert (const(corner, "kThreads"), const(corner, "kLdsBudget")) == \
        (fc.CORNER_THREADS, fc.CORNER_LDS_BUDGET)
    m = re.search(r"chunks = std::min\(\(n \+ (\d+)\) / (\d+), std::max\(1ll, (\d+) / tiles\)\)",
                  corner)
    assert m and int(m.group(1)) + 1 == int(m.group(2)) == fc.CORNER_PER_CHUNK
    assert int(m.group(3)) == fc.CORNER_GRID


#      id      tiles a walker, tiles, tiles a workgroup, workgroups, tiles of the last one,
#              workgroups whose tiles are of two walkers
COV_CLAIMS = {
    "2049x1": (1, 2049, 2, 1025, 1, 1024),        # every workgroup of two tiles
    "cp4": (1, 2100, 2, 1050, 2, 1050),
    "template256": (2, 2060, 2, 1030, 2, 0),      # a workgroup is a walker
    "straddle64": (3, 3000, 2, 1500, 2, 500),     # every third: tiles 2 and 3 of 0 .. 5
    "three64": (5, 5500, 3, 1834, 1, 733),        # two in five
}


@pytest.mark.parametrize("case", list(fc.COV))
def test_covariance_shapes_take_several_tiles_a_workgroup(case):
    W, N, ncols, tile = fc.COV[case]
    p = fc.cov_plan(W, N, tile)
    tpw, tiles, chunk, wgs, last, straddle = COV_CLAIMS[case]
    assert (p["tpw"], p["tiles"], p["chunk"], p["wgs"], p["last"]) == \
        (tpw, tiles, chunk, wgs, last), p
    assert p["tiles"] > fc.COV_MAX_SLOTS and p["chunk"] >= 2
    assert p["straddle"] == straddle, p
    assert 1 <= ncols <= 24


def test_covariance_columns_and_ragged_tiles():
    """cp4 is the CP = 4 kernel; template256's second tile has 44 rows, straddle64's third 2,
    three64's fifth 1."""
    assert (fc.COV["cp4"][2] + 3) // 4 * 4 == 4
    assert fc.COV["template256"][1] - 256 == 44
    assert fc.COV["straddle64"][1] - 2 * 64 == 2 and fc.COV["three64"][1] - 4 * 64 == 1
    assert fc.COV_PIPE == fc.COV["three64"] and fc.COV_PIPE[3] == "64"


def test_covariance_bad_rows_sit_where_the_pipeline_turns():
    W, N, ncols, tile = fc.COV_PIPE
    p = fc.cov_plan(W, N, tile)
    assert p["chunk"] == 3                                # the parity flips twice
    (first, second, third, ragged), gone = fc.cov_bad_rows(p, W, N)
    assert fc.cov_tile(p, *first)[1] == 0
    g2, k2, r2 = fc.cov_tile(p, *second)
    g3, k3, r3 = fc.cov_tile(p, *third)
    assert g2 == g3 and (k2, k3) == (1, 2) and r2 == r3
    assert ragged[1] == N - 1 and N % p["tile"] == 1 and fc.cov_tile(p, *ragged)[2] == 0
    walkers = {first[0], second[0], third[0], ragged[0], gone}
    assert len(walkers) == 4 and second[0] == third[0] and 0 not in walkers   # row 0: the pivot
    # the single-tile path of the bit-for-bit comparison: objects of so many walkers
    per = fc.COV_MAX_SLOTS // p["tpw"]
    assert fc.cov_plan(per, N, tile)["chunk"] == 1 and fc.cov_plan(per + 1, N, tile)["chunk"] == 2


def test_covariance_device_chain_shape():
    W, N, tile = fc.COV_CHAIN
    p = fc.cov_plan(W, N, tile)
    assert (p["tpw"], p["tiles"], p["chunk"]) == (3, 3300, 2) and p["straddle"] > 0


#      id            T, tiles a series, units, units a workgroup, workgroups, last
ACF_CLAIMS = {
    "1025x2": (512, 1, 1025, 2, 513, 1),
    "twopass": (512, 1, 1030, 2, 515, 2),
    "straddle64": (64, 3, 1800, 2, 900, 2),
    "five64": (64, 4, 4400, 5, 880, 5),
}


@pytest.mark.parametrize("case", list(fc.ACF))
def test_acf_shapes_take_several_units_a_workgroup(case):
    W, N, ncols, L, tile = fc.ACF[case]
    p = fc.acf_plan(W, N, ncols, L, tile)
    assert (p["T"], p["tiles"], p["units"], p["chunk"], p["wgs"], p["last"]) == ACF_CLAIMS[case], p
    assert p["units"] > fc.ACF_MAX_SLOTS and p["chunk"] >= 2
    if case == "twopass":
        assert L > 512                                    # acf_fold_kernel<2>
    if case == "straddle64":
        assert p["straddle"] == p["wgs"] // 3             # units 2 and 3 of every 0 .. 5
    if case == "five64":
        assert p["straddle"] == p["wgs"]                  # five units, four to a series


def test_acf_unused_series_cover_the_skip():
    W, N, ncols, L, tile = fc.ACF_SKIP
    assert fc.ACF_SKIP == fc.ACF["five64"]
    p = fc.acf_plan(W, N, ncols, L, tile)
    used = fc.acf_unused(p, set(fc.ACF_BAD_SERIES))
    assert all(len(u) == 5 for u in used)
    none = [g for g, u in enumerate(used) if not any(u)]
    assert none == [8]                                    # series 10 and the first tile of 11
    assert used[9] == [False, False, False, True, True]   # begins unused, ends used
    assert used[16] == [True, True, True, True, False]    # ends unused
    assert used[17] == [False, False, False, True, True]


def test_select_and_reduction_sizes_pass_the_grids():
    n = {k: fc.cdiv(v, w) * w for k, (v, w) in fc.PHOT.items()}     # whole rows of W samples
    assert fc.trips(n["cap"], fc.SEL_THREADS) == (1, 1)
    assert fc.trips(n["cap+1"], fc.SEL_THREADS) == (1, 2)
    assert fc.trips(n["third_trip"], fc.SEL_THREADS) == (2, 3)
    assert fc.PHOT["cap"][0] == fc.SEL_THREADS and fc.PHOT["cap+1"][0] == fc.SEL_THREADS + 1
    assert fc.cdiv(n["partials257"], fc.REDUCE_CHUNK) == 257 > fc.REDUCE_THREADS
    assert fc.cdiv(n["third_trip"], fc.REDUCE_CHUNK) <= fc.REDUCE_THREADS
    W, rows, _ = fc.ASTROM["700x400"]
    assert fc.SEL_THREADS < W * rows <= fc.CORRECT_THREADS
    W, rows, _ = fc.ASTROM["1025x1024"]
    assert W * rows == 1049600 > fc.CORRECT_THREADS
    assert fc.cdiv(W * rows, fc.REDUCE_CHUNK) == 257 > fc.REDUCE_THREADS


def test_corner_sizes_pass_the_piece_and_the_chunk_cap():
    n, ncols, nb2, nb1 = fc.CORNER_PIECES
    assert fc.CORNER_STAGE < n < 2 * fc.CORNER_STAGE and n - fc.CORNER_STAGE == 513
    n, ncols, nb2, nb1 = fc.CORNER_CHUNKS
    tiles = fc.corner_tiles(ncols, nb2, nb1)
    assert tiles == 138                                   # 276 pairs, two a tile
    want, cap, chunks = fc.corner_plan(n, tiles)
    assert (want, cap) == (15, 14) and 1 < chunks <= cap
    assert (n - 1) % fc.CORNER_THREADS == 0
    smaller = n - fc.CORNER_THREADS                       # the next smaller n of that form
    w2, c2, _ = fc.corner_plan(smaller, tiles)
    assert w2 <= c2
    assert n <= fc.CORNER_STAGE                           # one piece: the cap alone is crossed
