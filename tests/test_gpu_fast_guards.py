"""The FAST guards at their edges: which sweep a parameter vector gets, and what that
sweep computes there.

olpe_device.h chooses between FAST3, FAST2, the V-table sweep and the exact sweep with
fast3_fails / fast3_cols_pass / fast3_amp_ok (fast3_ok below 65 columns) and fast_level.
``guard_state`` restates their quantities in NumPy from the header's definitions; with it
each case places a PAIR of parameter vectors on a synthetic frame, one 0.2 % inside one
limit and one 0.2 % outside, everything else well clear of its limit.  Per pair:
 (a) the guard probe's verdict (tests/c/device_probe.hip: the device functions on the
     FAST model descriptor) equals the restatement's for both members, and the members
     differ in exactly the Gaussians and the comparison the case is about.  From the
     verdict follows the sweep: in the samplers of n <= 64 fast3_fails alone decides
     FAST3; in the samplers of wider cutouts and in the evaluation kernel at every n
     (olpe_model, olpe_chi2_batch) a failing Gaussian may still pass by its columns --
     so the outside member of a whole-grid Qb pair at 64 x 64 leaves FAST3 in the
     sampler, part (c), and keeps it in part (b); each case prints both;
 (b) olpe_model / olpe_chi2_batch of both members are within the tolerances of
     tests/test_gpu_parity.py of the oracle, FAST and EXACT;
 (c) 8 walkers x 150 iterations from the inside member follow the oracle (chains within
     10 x the FAST trajectory tolerance, identical accept decisions), and the traced
     proposals fell on both sides of the limit at least 10 times.
"""
import functools

import numpy as np
import pytest

import probe_lib as P
from oracle import olpe_oracle as ora

pytestmark = pytest.mark.gpu

TOL = {"exact": dict(model=1e-13, chi=1e-12, traj=1e-10),
       "fast": dict(model=1e-12, chi=1e-11, traj=1e-9)}      # tests/test_gpu_parity.py
GAP = 2e-3                      # each member's distance from the limit, relative
CLEAR = 1e-2                    # every other comparison's least distance from its limit
PI4 = 0.78539816339744830962

LAYOUT = {2: dict(sx=(0, 2), sy=(1, 3), sa=(6, 7), DX=4, DY=5, RATIO=8, OFF=9,
                  S1X=10, S1Y=11, S2X=12, S2Y=13, T1=14, T2=15, NP=16),
          3: dict(sx=(0, 2, 4), sy=(1, 3, 5), sa=(8, 9, 10), DX=6, DY=7, RATIO=11, OFF=12,
                  S1X=13, S1Y=14, S2X=15, S2Y=16, T1=17, T2=18, NP=19)}


# ----------------------------------------------------------------------------------
# The guards, restated (olpe_device.h: make_trig<true>, coef_inv, make_model, fast3_fails,
# fast3_cols_pass, fast3_amp_ok, fast_level)
# ----------------------------------------------------------------------------------
def row_stride(n):
    return 1 if n >= 64 else 64 // n


def descriptor(p, nsrc):
    """(amp, x0, y0, a, b, c), one entry per Gaussian g = 2 s (wide), 2 s + 1 (narrow)."""
    L = LAYOUT[nsrc]

    def coef(sx, sy, th):
        s, c = np.sin(th), np.cos(th)
        ix, iy = 1.0 / (sx * sx), 1.0 / (sy * sy)
        return (0.5 * (c * c * ix + s * s * iy), 0.5 * (2.0 * (s * c) * (ix - iy)),
                0.5 * (s * s * ix + c * c * iy))
    with np.errstate(all="ignore"):
        C1 = coef(p[L["S1X"]], p[L["S1Y"]], p[L["T1"]])
        C2 = coef(p[L["S2X"]], p[L["S2Y"]], p[L["T2"]])
    out = []
    for s in range(nsrc):
        tot = p[L["sa"][s]] - p[L["OFF"]]
        wide = tot * p[L["RATIO"]]
        xc, yc = p[L["sx"][s]], p[L["sy"][s]]
        out.append((wide, xc + p[L["DX"]], yc + p[L["DY"]]) + C2)
        out.append((tot - wide, xc, yc) + C1)
    return np.array(out, np.float64).T


def guard_state(p, n, nsrc):
    """The guards' verdict for parameter vector p at cutout size n, and the signed
    relative margin of every comparison per Gaussian (positive: the comparison holds).
    S = row_stride(n), rows0 = ceil(n / S), kc = rows0 // 2, km = max(kc, rows0-1-kc) + 1."""
    amp, x0, y0, a, b, c = descriptor(p, nsrc)
    G = 2 * nsrc
    S = row_stride(n)
    rows0 = -(-n // S)
    kc = rows0 // 2
    km = max(kc, rows0 - 1 - kc) + 1
    hi = n - 1.0
    with np.errstate(all="ignore"):
        mx = np.maximum(np.abs(x0), np.abs(hi - x0))
        my = np.maximum(np.abs(y0), np.abs(hi - y0))
        B = np.abs(b) * mx * my
        Qb = (a * (mx * mx) + B) + c * (my * my)
        cs = c * (S * S)
        row = cs * km * km
        K = cs * (kc * (kc + 1.0))
        fin = np.isfinite(Qb) & np.isfinite(amp) & (a >= 0) & (c >= 0)
        fails = ~((row < 600.0) & (Qb < 700.0 + K) & fin)
        # per column: lanes = S row groups x the columns of the grid
        j = np.arange(n, dtype=np.float64)[None, None, :]
        yr = np.arange(S, dtype=np.float64)[None, :, None]
        A_, B_, C_ = a[:, None, None], b[:, None, None], c[:, None, None]
        xd = j - x0[:, None, None]
        yd = yr - y0[:, None, None]
        bx = B_ * xd
        q0 = (A_ * (xd * xd) + bx * yd) + C_ * (yd * yd)
        d0 = bx * S + (C_ * S) * (2.0 * yd + S)
        xe = K[:, None, None] - q0
        xr = d0 + 2.0 * cs[:, None, None] * kc
        amin = a - (b * b) / (4.0 * c)
        ax2 = amin[:, None, None] * (xd * xd)
        colok = (np.abs(xr) < 170.0) & ((xe > -700.0) | (ax2 >= 100.0))
        cpass = ((row < 600.0) & (a >= 0) & (c > 0) & np.isfinite(amin) &
                 colok.reshape(G, -1).all(axis=1))
        ampok = np.abs(amp) < 1e20
        fin2 = np.isfinite(a) & np.isfinite(c) & np.isfinite(amp) & (a >= 0) & (c >= 0)
        ok1 = bool(np.all(fin2 & (B < 300.0)))
        ok2 = bool(np.all(fin2 & (Qb < 690.0)))
        big = np.full_like(xe, np.inf)
        margins = dict(
            row=(600.0 - row) / 600.0,
            qb=(700.0 + K - Qb) / (700.0 + K),
            xr=(170.0 - np.abs(xr).reshape(G, -1).max(axis=1)) / 170.0,
            # xe where the column is not excused by amin dx^2 >= 100, and the reverse
            xe=np.where(ax2 >= 100.0, big, (xe + 700.0) / 700.0).reshape(G, -1).min(axis=1),
            amin=np.where(xe > -700.0, big, (ax2 - 100.0) / 100.0).reshape(G, -1).min(axis=1),
            amp=(1e20 - np.abs(amp)) / 1e20,
            cross=(300.0 - B) / 300.0,
            q2=(690.0 - Qb) / 690.0)
    bits = lambda m: int(sum(1 << g for g in range(G) if m[g]))
    f = bits(fails)
    st = dict(fails=f, cpass=bits(cpass & fails), amp_ok=int(np.all(ampok | ~fails)),
              level=2 if ok2 else (1 if ok1 else 0), margins=margins)
    # who takes FAST3: the sampler kernels of n <= 64 (NT = n) test the whole grid only
    # (fast3_ok); the samplers of wider cutouts and, at every n, the evaluation kernel
    # behind olpe_model / olpe_chi2_batch (NT = 0) let a Gaussian that fails it pass by
    # its columns (fast3_cols_pass / fast3_ok_cols, with the amplitude bound)
    st["fast3_eval"] = (f & ~st["cpass"]) == 0 and bool(st["amp_ok"])
    st["fast3"] = st["fast3_eval"] if n > 64 else f == 0
    return st


def sweep_name(st, eval_kernel):
    """The sweep the restatement expects for a vector: in a sampler or in the evaluation
    kernel (which has room for the V table at every shape)."""
    if st["fast3_eval" if eval_kernel else "fast3"]:
        return "FAST3"
    return {2: "FAST2", 1: "V-table or exact", 0: "exact"}[st["level"]]


def verdict(st):
    return (st["fails"], st["cpass"], st["amp_ok"], st["level"])


# ----------------------------------------------------------------------------------
# Cases
# ----------------------------------------------------------------------------------
def base_vector(n, nsrc, near=False):
    """The synthetic truth (olpefit_amd.synth) plus the chi^2 slot; near: the companion
    and the third source a few pixels from the primary, so that at n <= 64, where only
    the whole-grid guard runs, every narrow Gaussian passes it at small sigma."""
    from olpefit_amd import synth
    p = np.append(synth.truth_params(n, nsrc), 0.0)
    if near:
        L = LAYOUT[nsrc]
        off = ((0.8, -0.6), (-0.6, -1.2))
        for s in range(1, nsrc):
            p[L["sx"][s]] = p[L["sx"][0]] + off[s - 1][0]
            p[L["sy"][s]] = p[L["sy"][0]] + off[s - 1][1]
    return p


def _solve(f, target, lo, hi):
    """t in [lo, hi] with f(t) = target by bisection (f monotonic on the bracket)."""
    flo = f(lo) - target
    assert flo * (f(hi) - target) < 0, (f(lo), f(hi), target)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if (f(mid) - target) * flo > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


W_TRAJ, IT_TRAJ = 8, 150
# Walker seeds per case (default 900..907).  The synthetic frames pull a narrow core back
# to the truth's width, so from most seeds a walker leaves the row-step limit for good
# within a few steps; these are the seeds, of 900..1027, whose oracle trajectories propose
# on the far side most often (checked on the CPU with the restatement).
SEEDS = {
    "row-narrow-64x2": (947, 954, 965, 989, 996, 1002, 1009, 1021),
    "row-wide-64x2": (920, 921, 929, 936, 942, 979, 1017, 1018),
    "row-narrow-64x3": (928, 941, 965, 980, 991, 998, 1016, 1019),
    "row-narrow-128x3": (918, 928, 933, 941, 944, 948, 950, 957),
    "row-rot-128x3": (924, 925, 926, 928, 933, 941, 947, 948),
    "row-wide-128x3": (903, 922, 940, 942, 955, 956, 957, 959),
}


class Case:
    """make(t) -> parameter vector; the pair is where margin `name` of Gaussian g is
    +GAP (inside) and -GAP (outside).  bits: the Gaussians whose verdict may differ
    between the members; variants: environment settings of the trajectory runs."""

    def __init__(self, cid, n, nsrc, make, name, g, lo, hi, bits, variants, levels=None,
                 seeds=None, clear=CLEAR):
        self.id, self.n, self.nsrc, self.make, self.name, self.g = cid, n, nsrc, make, name, g
        self.lo, self.hi, self.bits, self.variants, self.levels = lo, hi, bits, variants, levels
        self.seeds = tuple(seeds or SEEDS.get(cid, range(900, 900 + W_TRAJ)))
        self.clear = clear

    def margin(self, p):
        return guard_state(p, self.n, self.nsrc)["margins"][self.name][self.g]

    @functools.lru_cache(maxsize=None)
    def pair(self):
        f = lambda t: self.margin(self.make(t))
        return (self.make(_solve(f, GAP, self.lo, self.hi)),
                self.make(_solve(f, -GAP, self.lo, self.hi)))


def _set(p, **kw):
    p = p.copy()
    for k, v in kw.items():
        p[int(k[1:])] = v
    return p


def _cases():
    cases = []
    RING = ({}, {"OLPE_RING": "0"})
    WPB = ({"OLPE_WPB": "12"}, {"OLPE_WPB": "16"})
    ONE = ({},)          # (16 waves of the 3-source 64x64 sampler do not fit the LDS)
    for n, nsrc in ((32, 2), (40, 2), (64, 2), (64, 3), (128, 3)):
        L = LAYOUT[nsrc]
        var = RING if n == 128 else WPB if (n, nsrc) == (64, 2) else ONE
        b = base_vector(n, nsrc, near=n <= 64)
        odd = sum(2 << (2 * s) for s in range(nsrc))
        even = sum(1 << (2 * s) for s in range(nsrc))
        tag = f"{n}x{nsrc}"

        def circ_narrow(t, b=b, L=L):
            p = b.copy()
            p[L["S1X"]] = p[L["S1Y"]] = t
            p[L["T1"]] = 0.0
            return p

        def circ_wide(t, b=b, L=L):
            p = b.copy()
            p[L["S2X"]] = p[L["S2Y"]] = t
            p[L["T2"]] = 0.0
            return p

        def rot_narrow(t, b=b, L=L):
            p = b.copy()
            p[L["S1Y"]], p[L["S1X"]], p[L["T1"]] = t, 1.15 * t, 0.6
            return p
        cases.append(Case(f"row-narrow-{tag}", n, nsrc, circ_narrow, "row", 1, 0.2, 4.0, odd, var))
        cases.append(Case(f"row-wide-{tag}", n, nsrc, circ_wide, "row", 0, 0.2, 4.0, even, var))
        # (the rotated set at 128: sources near the centre, or the third one's cross term
        # fails its columns on both sides of the row-step limit)
        cases.append(Case(f"row-rot-{tag}", n, nsrc,
                          functools.partial(rot_narrow, b=base_vector(n, nsrc, near=True)),
                          "row", 1, 0.2, 4.0, odd, var))
    # Qb = 700 + c S^2 kc (kc + 1): narrow sigma 10 % above the row-step limit, the
    # companion's y moved toward the edge
    for nsrc in (2, 3):
        L = LAYOUT[nsrc]
        b = base_vector(64, nsrc, near=True)
        s0 = 1.1 * 33.0 / np.sqrt(1200.0)
        b[L["S1X"]] = b[L["S1Y"]] = s0
        b[L["T1"]] = 0.0

        def comp_y(t, b=b, L=L):
            p = b.copy()
            p[L["sy"][1]] = t
            return p
        cases.append(Case(f"qb-64x{nsrc}", 64, nsrc, comp_y, "qb", 3, 5.0, 30.0, 1 << 3,
                          WPB if nsrc == 2 else ONE))
    # the per-column limits (128 columns; the tested source is the last one: the third
    # source, or the companion of the 2-source model), moved off-centre
    for nsrc in (3, 2):
        L = LAYOUT[nsrc]
        k = nsrc - 1
        g = 2 * k + 1
        b = base_vector(128, nsrc)
        ix, iy = L["sx"][k], L["sy"][k]
        # |xr| = 170: b dx dominates, so a thin core (0.25 x 3 px) turned by 0.1 rad and
        # the source's x moved away from the centre
        bx = _set(b, **{f"i{L['S1X']}": 0.25, f"i{L['S1Y']}": 3.0, f"i{L['T1']}": 0.1,
                        f"i{iy}": 45.0})
        cases.append(Case(f"xr-128x{nsrc}", 128, nsrc,
                          lambda t, bx=bx, ix=ix: _set(bx, **{f"i{ix}": t}),
                          "xr", g, 2.0, 60.0, 1 << g, RING))
        # xe = -700: the truth's core, the source's y moved toward the top edge; its x on
        # a half pixel so that no column's amin dx^2 is near 100
        be = _set(b, **{f"i{ix}": np.floor(b[ix]) + 0.5})
        cases.append(Case(f"xe-128x{nsrc}", 128, nsrc,
                          lambda t, be=be, iy=iy: _set(be, **{f"i{iy}": t}),
                          "xe", g, 70.0, 120.0, 1 << g, RING))
        # amin dx^2 = 100: a core of 0.5277 x 2.2 px (a = 1.7956: dx = 7.5 gives 101), the
        # source so high that a_0 underflows (xe <= -700) from a dx^2 = 87.5 on, its x
        # moved off the half pixel until the column 7.5 - t away reaches 100
        sx1, sy1 = np.sqrt(0.5 / 1.7956), 2.2
        c1 = 0.5 / (sy1 * sy1)
        y0 = np.sqrt((700.0 + c1 * 64.0 * 65.0 - 87.5) / c1)
        ba = _set(b, **{f"i{L['S1X']}": sx1, f"i{L['S1Y']}": sy1, f"i{L['T1']}": 0.0,
                        f"i{iy}": y0})
        x_half = np.floor(b[ix]) + 0.5
        cases.append(Case(f"amin-128x{nsrc}", 128, nsrc,
                          lambda t, ba=ba, ix=ix, xh=x_half: _set(ba, **{f"i{ix}": xh - t}),
                          "amin", g, 0.0, 0.2, 1 << g, RING))
    # |A| = 1e20: the third source 100 px left of the frame, so that its Gaussians fail
    # the whole-grid test and pass their columns through amin dx^2 >= 100 with an a_0
    # that underflows -- what the amplitude bound is for: A e^-100 must stay negligible.
    # Its amplitude raised; on the frame the source is below 1e-30, so chi^2 stays
    # moderate and the accept decisions meaningful.
    L = LAYOUT[3]
    b = base_vector(128, 3)
    b[L["sx"][2]] = -100.0
    cases.append(Case("amp-128x3", 128, 3,
                      lambda t, b=b, i=L["sa"][2]: _set(b, **{f"i{i}": t}),
                      "amp", 5, 1e19, 1e21, 1 << 5, RING))
    # the same limit with the source on the frame, where the 1e20 Gaussian dominates the
    # model: chi^2 is ~1e40, finite, and no accept decision means anything at that size
    # (a chi^2 difference is far below one rounding of the sum), so verdict and
    # evaluation only -- no variants, no trajectory
    b = base_vector(128, 3)
    cases.append(Case("amp-onframe-128x3", 128, 3,
                      lambda t, b=b, i=L["sa"][2]: _set(b, **{f"i{i}": t}),
                      "amp", 5, 1e19, 1e21, 1 << 5, ()))
    # the fallbacks' own limits, with a core so small that FAST3 is refused (row step)
    for n, var in ((64, WPB), (40, ONE)):
        L = LAYOUT[2]
        b = base_vector(n, 2)
        # B = |b| mx my = 300 (kFastCross): a 0.4 x 0.5 px core, theta bisected
        bc = _set(b, **{f"i{L['S1X']}": 0.4, f"i{L['S1Y']}": 0.5})
        cases.append(Case(f"cross-{n}x2", n, 2,
                          lambda t, bc=bc, i=L["T1"]: _set(bc, **{f"i{i}": t}),
                          "cross", 3, 0.005, 0.4, 1 << 3, var, levels=(1, 0)))
        # Qb = 690 (kFast2Q): c 1.2 % above the row-step limit (sigma_y 0.95 px at 64,
        # 0.60 px at 40), sigma_x 3 px, the primary on the grid centre, the companion
        # beside it, its y bisected
        km = n // 2 + 1
        syl = km / np.sqrt(1200.0) / 1.006
        ctr = 0.5 * (n - 1)
        bq = _set(b, **{f"i{L['S1X']}": 3.0, f"i{L['S1Y']}": syl, f"i{L['T1']}": 0.0,
                        "i0": ctr, "i1": ctr, "i2": ctr + 0.8})
        cases.append(Case(f"q2-{n}x2", n, 2,
                          lambda t, bq=bq: _set(bq, i3=t),
                          "q2", 3, ctr, ctr + 6.0, 1 << 3, var, levels=(2, 1)))
    return cases


CASES = _cases()
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


@functools.lru_cache(maxsize=None)
def frame(n, nsrc):
    from olpefit_amd import synth
    img, _ = synth.make_image(n, nsrc, 3)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    return img, dm, err


def oracle_eval(p, n, nsrc):
    _, dm, err = frame(n, nsrc)
    with np.errstate(all="ignore"):
        m = ora.build_analytical_model(p, n, nsrc)
        return m, float(ora.chi_squared(dm, m, err))


def check_pair(case):
    """The conditions on a pair that need no GPU: the tested margin at +-GAP, every other
    margin clear, the verdicts differing only in the tested Gaussians, finite oracle."""
    pin, pout = case.pair()
    sts = [guard_state(p, case.n, case.nsrc) for p in (pin, pout)]
    G = 2 * case.nsrc
    for st, want in zip(sts, (GAP, -GAP)):
        got = st["margins"][case.name][case.g]
        assert abs(got - want) < 1e-6, (case.id, got)
        for name, m in st["margins"].items():
            for g in range(G):
                if name == case.name and (case.bits >> g) & 1:
                    assert abs(m[g] - want) < 2e-4 or abs(m[g]) > case.clear, (case.id, name, g, m[g])
                    continue
                # comparisons that decide nothing for this vector do not count: the
                # column tests of a Gaussian that passes the whole-grid test or fails the
                # row step (part of both tests); the level tests where every kernel takes
                # FAST3.  (At n <= 64 the column tests run in the evaluation kernel only.)
                if name in ("xr", "xe", "amin") and (not (st["fails"] >> g) & 1 or
                                                      st["margins"]["row"][g] < 0):
                    continue
                if name == "amp" and not (st["fails"] >> g) & 1:
                    continue
                if name == "qb" and case.n > 64:
                    continue          # decides only who takes the column test
                if name in ("cross", "q2") and case.levels is None:
                    continue
                assert abs(m[g]) > case.clear, (case.id, name, g, m[g])
    a, b = sts
    if case.levels is None:
        assert a["fast3"] and not b["fast3"], case.id
        diff = (a["fails"] ^ b["fails"]) | (a["cpass"] ^ b["cpass"])
        if case.name != "amp":
            assert diff and (diff & ~case.bits) == 0, (case.id, bin(diff))
            assert a["amp_ok"] == b["amp_ok"] == 1
        else:
            assert (a["amp_ok"], b["amp_ok"]) == (1, 0) and diff == 0
    else:
        assert not a["fast3"] and not b["fast3"], case.id
        assert verdict(a)[:3] == verdict(b)[:3]
        assert (a["level"], b["level"]) == case.levels, (case.id, a["level"], b["level"])
    for p in (pin, pout):
        m, chi = oracle_eval(p, case.n, case.nsrc)
        assert np.all(np.isfinite(m)) and np.isfinite(chi), case.id
    return sts


def side(case, p):
    """True where the tested comparison holds for vector p."""
    return guard_state(p, case.n, case.nsrc)["margins"][case.name][case.g] > 0.0


# ----------------------------------------------------------------------------------
# Tests
# ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_device_verdict_matches_restatement(lib_loaded, cid):
    """(a) The device guards put each member on the side the restatement does, and the
    members differ in exactly the tested Gaussians' bits (or the level)."""
    case = BY_ID[cid]
    sts = check_pair(case)
    got = P.guards(case.nsrc, case.n, np.array(case.pair()))
    for k, st in enumerate(sts):
        assert tuple(got[k]) == verdict(st), (cid, "inside" if k == 0 else "outside",
                                              tuple(got[k]), verdict(st))
    assert tuple(got[0]) != tuple(got[1])


@pytest.mark.parametrize("cid", IDS)
def test_evaluation_at_the_edge(lib_loaded, cid):
    """(b) Model and chi^2 of both members against the oracle, FAST and EXACT, at the
    tolerances of tests/test_gpu_parity.py; the worst model error is printed as a
    fraction of the tolerance (the table of DESIGN.md §5)."""
    from olpefit_amd.core import Sampler
    case = BY_ID[cid]
    img, _, _ = frame(case.n, case.nsrc)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=case.nsrc)
    fr = {}
    try:
        for side_name, p in zip(("inside", "outside"), case.pair()):
            ref, chi_ref = oracle_eval(p, case.n, case.nsrc)
            assert np.all(np.isfinite(ref)) and np.isfinite(chi_ref)
            for mode in ("fast", "exact"):
                s.set_eval_mode(mode)
                m = s.build_analytical_model(p)
                chi = s.chi_squared(p)
                em = np.max(np.abs(m - ref)) / np.max(np.abs(ref))
                ec = abs(chi - chi_ref) / abs(chi_ref)
                fr[side_name, mode] = (em / TOL[mode]["model"], ec / TOL[mode]["chi"])
    finally:
        s.close()
    sts = [guard_state(p, case.n, case.nsrc) for p in case.pair()]
    print(f"EDGE {cid}: sweeps of olpe_model {sweep_name(sts[0], True)} / "
          f"{sweep_name(sts[1], True)}, of the sampler {sweep_name(sts[0], False)} / "
          f"{sweep_name(sts[1], False)}; " + ", ".join(f"{k[0]} {k[1]} model {v[0]:.3f} chi {v[1]:.3f}"
                                      for k, v in fr.items()) + " (fractions of the tolerance)")
    for k, v in fr.items():
        assert v[0] <= 1.0 and v[1] <= 1.0, (cid, k, v)


# ----------------------------------------------------------------------------------
# Trajectories
# ----------------------------------------------------------------------------------


def start_vector(p, n, nsrc):
    p = np.array(p, np.float64)
    p[-1] = oracle_eval(p, n, nsrc)[1]
    return p


@functools.lru_cache(maxsize=None)
def oracle_run(n, nsrc, key, seeds):
    """The oracle's 8 walkers x 150 iterations from the start vector `key` (a tuple):
    chains, accept decisions, and per step the drawn index, the proposal and the value
    it replaces."""
    _, dm, err = frame(n, nsrc)
    p0 = np.array(key)
    chains, acc, r, new, cur = [], [], [], [], []
    for sd in seeds:
        wk = ora.Walker(dm, err, p0, sd, nsrc=nsrc)
        rows, a_, r_, n_, c_ = [], [], [], [], []
        for _ in range(IT_TRAJ):
            before = wk.parameters.copy()
            rec = wk.step()
            rows.append(wk.parameters.copy())
            r_.append(rec[0]); n_.append(rec[1]); a_.append(bool(rec[4])); c_.append(before[rec[0]])
        chains.append(rows); acc.append(a_); r.append(r_); new.append(n_); cur.append(c_)
    return (np.array(chains), np.array(acc), np.array(r), np.array(new), np.array(cur))


def proposals(p0, chain, r, new):
    """The proposal vectors of a run: the state before each step with parameter r
    replaced by the proposal."""
    prev = np.concatenate([np.broadcast_to(p0, (chain.shape[0], 1, chain.shape[2])),
                           chain[:, :-1]], axis=1).copy()
    w, i = np.indices(r.shape)
    cur = prev[w, i, r.astype(int)]
    prev[w, i, r.astype(int)] = new
    return prev, cur


def run_sampler(n, nsrc, p0, seeds, env, monkeypatch):
    from olpefit_amd.core import Sampler
    for k in ("OLPE_RING", "OLPE_WPB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    img, _, _ = frame(n, nsrc)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    try:
        s.set_eval_mode("fast")
        s.seed(np.array(seeds))
        s.set_state(np.tile(p0, (W_TRAJ, 1)))
        s.enable_trace(True)
        chain = s.run(IT_TRAJ, burn_in=0, record_stride=1)
        tr = s.trace(IT_TRAJ)
    finally:
        s.close()
    return chain, tr


def assert_follows_oracle(chain, tr, ref):
    ref_chain, ref_acc, ref_r = ref[:3]
    np.testing.assert_array_equal(tr[:, :, 0].astype(int), ref_r)
    np.testing.assert_array_equal(tr[:, :, 5] > 0.5, ref_acc)
    np.testing.assert_allclose(chain, ref_chain, rtol=10 * TOL["fast"]["traj"], atol=0)


TRAJ = [(c.id, k) for c in CASES for k in range(len(c.variants))]


@pytest.mark.parametrize("cid,k", TRAJ, ids=[f"{c}-{k}" for c, k in TRAJ])
def test_trajectories_cross_the_edge(lib_loaded, monkeypatch, cid, k):
    """(c) From the inside member, the FAST sampler of the shape (128 x 128: the ring
    sampler and OLPE_RING=0; 64 x 64 with two sources: 12 and 16 waves) follows the
    oracle, and its traced proposals lie on both sides of the limit >= 10 times each."""
    case = BY_ID[cid]
    p0 = start_vector(case.pair()[0], case.n, case.nsrc)
    ref = oracle_run(case.n, case.nsrc, tuple(p0), case.seeds)
    chain, tr = run_sampler(case.n, case.nsrc, p0, case.seeds, case.variants[k], monkeypatch)
    assert_follows_oracle(chain, tr, ref)
    props, _ = proposals(p0, chain, tr[:, :, 0], tr[:, :, 1])
    inside = np.array([side(case, q) for q in props.reshape(-1, props.shape[-1])])
    print(f"TRAJ {cid} {case.variants[k]}: {inside.sum()} proposals inside, "
          f"{(~inside).sum()} outside, {int(ref[1].sum())} accepted")
    assert inside.sum() >= 10 and (~inside).sum() >= 10


# ----------------------------------------------------------------------------------
# Seams: |theta| = pi/4 of make_trig<true>, |x| = 0.0625 of the log-normal proposal
# ----------------------------------------------------------------------------------
def seam_start(kind, n, nsrc):
    L = LAYOUT[nsrc]
    p = base_vector(n, nsrc)
    if kind == "theta":
        p[L["T1"]] = PI4 * (1.0 - 1e-3)
        p[L["T2"]] = -PI4 * (1.0 + 1e-3)
    return start_vector(p, n, nsrc)


SEAM_SEEDS = tuple(range(500, 500 + 8))


def seam_stats(p0, nsrc, r, new, cur):
    """Per run: theta proposals on either side of pi/4, and the log-normal exponents
    x = ln(new / cur) below, above and within 5 % of 0.0625."""
    L = LAYOUT[nsrc]
    t1, t2 = np.abs(new[r == L["T1"]]), np.abs(new[r == L["T2"]])
    lognorm = ora.layout(nsrc)[3]
    m = np.isin(r, lognorm)
    with np.errstate(all="ignore"):
        x = np.abs(np.log(new[m] / cur[m]))
    return dict(t1_in=int(np.sum(t1 <= PI4)), t1_out=int(np.sum(t1 > PI4)),
                t2_in=int(np.sum(t2 <= PI4)), t2_out=int(np.sum(t2 > PI4)),
                x_below=int(np.sum(x < 0.0625)), x_above=int(np.sum(x >= 0.0625)),
                x_near=int(np.sum(np.abs(x - 0.0625) <= 0.05 * 0.0625)))


@pytest.mark.parametrize("n,nsrc,env", [(64, 2, {"OLPE_WPB": "12"}), (64, 2, {"OLPE_WPB": "16"}),
                                        (128, 3, {}), (128, 3, {"OLPE_RING": "0"})],
                         ids=["64x2-wpb12", "64x2-wpb16", "128x3-ring", "128x3-noring"])
@pytest.mark.parametrize("kind", ["theta", "truth"])
def test_seam_runs(lib_loaded, monkeypatch, kind, n, nsrc, env):
    """Two runs of the same form (and the same sampler variants) across the seams of the
    FAST proposal path.  theta: both
    angles start 0.1 % from +-pi/4, so the theta proposals (widths 0.008 / 0.01 rad) take
    both branches of make_trig<true>, each angle on its own.  truth: every log-normal parameter starts at the
    synthetic truth.  In both, every log-normal proposal equals the oracle's of the same
    step within 1e-14 relative: the deviate is within 3.2e-15 of NumPy's, times
    w ln10 |g| <= 0.37 is 1.2e-15; the exponential (degree-9 Taylor polynomial below
    |x| = 0.0625, ExpTab above) <= 1.33 ulp = 3e-16 relative at most; the product one
    rounding, 1.1e-16; the oracle's own log10 / power ~1.5e-15; about 4e-15 in all, with
    2.5 x margin.  The runs draw on both sides of |x| = 0.0625 and within 5 % of it (the
    0.02-dex amplitude width at |g| = 1.36).  Coefficients of degree >= 8 of the
    polynomial stay below what this sees (x^8 / 8! = 6e-15 at the seam).
    Measured (MI355X): 1.35e-15."""
    p0 = seam_start(kind, n, nsrc)
    ref = oracle_run(n, nsrc, tuple(p0), SEAM_SEEDS)
    chain, tr = run_sampler(n, nsrc, p0, SEAM_SEEDS, env, monkeypatch)
    assert_follows_oracle(chain, tr, ref)
    r, new = tr[:, :, 0].astype(int), tr[:, :, 1]
    _, cur = proposals(p0, chain, r, new)
    err, x = P.lognormal_proposal_error(r, new, cur, ref[3], ref[4], ora.layout(nsrc)[3])
    st = seam_stats(p0, nsrc, r, new, cur)
    print(f"SEAM {kind} {n}x{nsrc} {env}: log-normal proposals max rel {err.max():.3e} over "
          f"{err.size}; {st}")
    assert err.max() <= 1e-14
    assert st["x_below"] >= 10 and st["x_above"] >= 10 and st["x_near"] >= 1
    if kind == "theta":
        assert min(st["t1_in"], st["t1_out"], st["t2_in"], st["t2_out"]) >= 3
