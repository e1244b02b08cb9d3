"""The shapes at which the step-3 fold objects give a workgroup (or a thread) more than one
unit of work, shared by the GPU tests that run them (test_gpu_covariance.py, test_gpu_acf.py,
test_gpu_photometry.py, test_gpu_astrometry.py, test_gpu_corner.py) and by
tests/test_fold_plans_cpu.py, which reads the caps from the sources and asserts that every
shape here still crosses them.  No GPU import.

Every fold caps its grid; below the cap a workgroup takes one unit and its loop runs once:

    cov_fold_kernel      2048 workgroups over W ceil(N / tile) tiles of one walker's rows
    acf_fold_kernel      1024 workgroups over series x ceil(N / T) time tiles
    select_*_kernel      1024 x 256 threads, grid-stride over the samples
    reduce_stage2_kernel 256 threads over the ceil(n / 4096) stage-1 partials (olpe_reduce.h:
                         astrometry, moments), as phot_reduce_stage2
    astrom_correct       4096 x 256 threads, grid-stride
    corner fold_rows     upload pieces of 2^18 samples
    corner launch_fold   at most 2048 / tiles chunks of the samples

The plan functions restate the few host lines that turn a shape into (units, units per
workgroup, workgroups); the constants below are the sources' (test_fold_plans_cpu.py
compares them).
"""

COV_MAX_SLOTS = 2048          # kMaxSlots, olpe_cov.hip
COV_DEFAULT_TILE = 256        # kDefaultTile
ACF_MAX_SLOTS = 1024          # kMaxSlots, olpe_acf.hip
ACF_SUB, ACF_MAX_TILE, ACF_MAX_GROUP = 64, 512, 16      # kSub, kMaxTile, kMaxGroup
ACF_LDS_BUDGET = 79 * 1024    # kLdsBudget
SEL_THREADS = 1024 * 256      # kSelBlocks x kSelThreads, olpe_select.h
REDUCE_CHUNK = 256 * 16       # kThreads x kPer: samples per stage-1 partial (phot, astrom)
REDUCE_THREADS = 256          # kThreads: stage 2 is one workgroup of them
CORRECT_THREADS = 4096 * 256  # cgrid's cap x kThreads, olpe_astrom.hip
CORNER_STAGE = 1 << 18        # kStageSamples, olpe_corner.hip
CORNER_PER_CHUNK, CORNER_GRID = 4096, 2048      # launch_fold, olpe_corner.hip
CORNER_THREADS, CORNER_LDS_BUDGET = 512, 64 * 1024


def cdiv(a, b):
    return -(-a // b)


def slots(units, cap):
    """(units per workgroup, workgroups) of launch_fold in olpe_cov.hip and olpe_acf.hip."""
    s = min(units, cap)
    chunk = cdiv(units, s)
    return chunk, cdiv(units, chunk)


# ------------------------------------------------------------------------- covariance
# id -> (W, N, ncols, OLPE_COV_TILE or None)
COV = {
    "2049x1": (2049, 1, 17, None),        # 2 tiles a workgroup, two walkers each; last has one
    "cp4": (2100, 3, 2, None),            # the CP = 4 instantiation
    "template256": (1030, 300, 20, None),  # <CP, 256>, a ragged second tile of 44 rows
    "straddle64": (1000, 130, 17, "64"),  # 3 tiles a walker: every third workgroup straddles
    "three64": (1100, 257, 24, "64"),     # 5 tiles a walker, 3 a workgroup, the parity flips twice
}
COV_PIPE = COV["three64"]                  # the non-finite and the bit-for-bit tests
COV_CHAIN = (1100, 130, "64")              # fold(sampler): W, rows, tile (PS = 17)


def cov_plan(W, N, tile=None, max_slots=COV_MAX_SLOTS):
    """The fold of W walkers of N rows, per-walker form (pooled, the rows are one walker of
    W N rows)."""
    tile = int(tile or COV_DEFAULT_TILE)
    tpw = cdiv(N, tile)
    tiles = W * tpw
    chunk, wgs = slots(tiles, max_slots)
    return {"tile": tile, "tpw": tpw, "tiles": tiles, "chunk": chunk, "wgs": wgs,
            "last": tiles - (wgs - 1) * chunk,                 # tiles of the last workgroup
            "straddle": sum(1 for g in range(wgs)
                            if (g * chunk) // tpw != (min(tiles, (g + 1) * chunk) - 1) // tpw)}


def cov_tile(plan, w, row):
    """(workgroup, position in its chunk, row within the tile) of row `row` of walker w."""
    q = w * plan["tpw"] + row // plan["tile"]
    return q // plan["chunk"], q % plan["chunk"], row % plan["tile"]


def cov_bad_rows(plan, W, N):
    """Where the non-finite rows go on COV_PIPE, from the plan: [(walker, row)] for the first
    tile of a chunk, the second and third tile of one chunk at one row index, a walker's
    ragged last tile; and the walker that loses every row."""
    tpw, chunk, tile = plan["tpw"], plan["chunk"], plan["tile"]
    assert chunk >= 3 and N % tile
    at = lambda q, r: (q // tpw, (q % tpw) * tile + r)
    first = at(7 * chunk, 5)
    # a chunk whose second and third tile are whole tiles of one walker
    g = next(g for g in range(100, plan["wgs"])
             if (g * chunk + 1) // tpw == (g * chunk + 2) // tpw
             and (g * chunk + 2) % tpw != tpw - 1)
    second, third = at(g * chunk + 1, 17), at(g * chunk + 2, 17)
    ragged = (200, N - 1)
    return [first, second, third, ragged], 500


# --------------------------------------------------------------------- autocorrelation
# id -> (W, N, ncols, L, OLPE_ACF_TILE or None)
ACF = {
    "1025x2": (1025, 2, 17, 64, None),    # one tile a series, 2 units a workgroup, last has one
    "twopass": (1030, 70, 3, 1024, None),  # NP = 2
    "straddle64": (600, 130, 17, 64, "64"),   # 3 tiles a series, 2 units a workgroup
    "five64": (1100, 200, 17, 64, "64"),  # 4 tiles a series, 5 units a workgroup
}
ACF_SKIP = ACF["five64"]
ACF_BAD_SERIES = (10, 11, 21)             # see acf_unused


def acf_tile(ncols, L, tile=None):
    """plan() of olpe_acf.hip: the time tile's rows."""
    skew = lambda i: i + 2 * (i >> 3)
    best, best_t = None, 0
    for T in range(ACF_SUB, ACF_MAX_TILE + 1, ACF_SUB):
        if tile and T != int(tile):
            continue
        G = min(ncols, ACF_MAX_GROUP, ACF_LDS_BUDGET // ((skew(T + L) + 2) * 8))
        if G < 1:
            continue
        groups = cdiv(ncols, G)
        score = groups * (T + L) / T
        if not best_t or score <= best:
            best, best_t = score, T
    return best_t


def acf_plan(W, N, ncols, L, tile=None, max_slots=ACF_MAX_SLOTS):
    T = acf_tile(ncols, L, tile)
    tiles = cdiv(N, T)
    units = W * tiles
    chunk, wgs = slots(units, max_slots)
    return {"T": T, "tiles": tiles, "units": units, "chunk": chunk, "wgs": wgs,
            "last": units - (wgs - 1) * chunk,
            "straddle": sum(1 for g in range(wgs)
                            if (g * chunk) // tiles != (min(units, (g + 1) * chunk) - 1) // tiles)}


def acf_unused(plan, bad):
    """Per workgroup the used flags of its units, in unit order, with the series `bad` unused."""
    chunk, tiles, units = plan["chunk"], plan["tiles"], plan["units"]
    return [[(u // tiles) not in bad for u in range(g * chunk, min(units, (g + 1) * chunk))]
            for g in range(plan["wgs"])]


# ------------------------------------------------- order statistics and the reductions
# id -> (values, walkers of the chain): the samples are padded to whole rows of W
PHOT = {"cap": (262144, 64), "cap+1": (262145, 64), "third_trip": (600001, 64),
        "partials257": (1048577, 1024)}
# id -> (walkers, rows, with tables)
ASTROM = {"700x400": (700, 400, True), "1025x1024": (1025, 1024, True)}


def trips(n, threads):
    """(fewest, most) trips a thread of a grid-stride loop over n samples makes."""
    return n // threads, cdiv(n, threads)


# ---------------------------------------------------------------------- corner histograms
CORNER_PIECES = ((1 << 18) + 513, 5, 9, 100)       # samples, columns, bins, fine bins
CORNER_CHUNKS = (57345, 24, 64, 4096)


def corner_tiles(ncols, nb2, nb1):
    """max(ntiles1, ntiles2) of olpe_corner_create."""
    npairs = ncols * (ncols - 1) // 2
    cmax = min(ncols, CORNER_LDS_BUDGET // (nb1 * 4))
    cpt = cdiv(ncols, cdiv(ncols, cmax))
    lds2 = lambda ppt: (ncols * (nb2 + 1) * 8 + ncols * 16 + ppt * ((nb2 * nb2) | 1) * 4
                        + ((ppt + 3) & ~3) * 2 + ncols * (CORNER_THREADS + 4))
    pmax = 1
    while pmax < npairs and lds2(pmax + 1) <= CORNER_LDS_BUDGET:
        pmax += 1
    ppt = cdiv(npairs, cdiv(npairs, pmax))
    return max(cdiv(ncols, cpt), cdiv(npairs, ppt))


def corner_plan(n, tiles):
    """(chunks asked for, cap on them, chunks launched) of launch_fold in olpe_corner.hip."""
    want, cap = cdiv(n, CORNER_PER_CHUNK), max(1, CORNER_GRID // tiles)
    chunk = cdiv(n, min(want, cap))
    chunk = cdiv(chunk, CORNER_THREADS) * CORNER_THREADS
    return want, cap, cdiv(n, chunk)
