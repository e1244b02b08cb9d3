"""NumPy restatement of the reference's astrometry, line by line (test helper; the
comparison reference of tests/test_gpu_astrometry.py).

``restate2``: apf_step3.py:211-256, :283-343, :401-450.  ``restate3``:
3body/apf_step3_3body.py:247-288, :315-390, :450-518.  Both take the collated chains
[rows, walkers, PS] (what :169-205 builds, as step3.load_chains returns it), the scalars
the reference reads from the header (olpefit_amd.astrometry.header_scalars) and the two
inputs this build takes from the caller: the distortion tables (None: no correction) and
``deltaR`` (:391).  Statement order and operand order are the reference's.
"""
import numpy as np


def _dedistort(x, y, x_dist, y_dist, xdiff, ydiff):
    """:234-253 for one source: positions already + 1 (:211-214)."""
    if x_dist is None:
        return x, y
    x_int = np.int_(x)                                   # :234-237
    y_int = np.int_(y)
    x_int = x_int + xdiff                                # :244-247
    y_int = y_int + ydiff
    return x + x_dist[y_int, x_int], y + y_dist[y_int, x_int]   # :250-253


def _pa(deltax, deltay, s, variant):
    """:290-341 (3body compute_pa :330-387)."""
    pa = np.arctan2(-deltax, deltay)                     # :290
    pa = np.degrees(pa)                                  # :291
    if variant == 3:
        pa = pa % 360                                    # 3body :334
    pa = pa + s["rotation_angle"]                        # :304
    if s["use_rotcorr"]:
        pa = pa + s["rotcorr"]                           # :337
    added = False
    if np.mean(pa) < 0:                                  # :340-341
        pa = pa + 360.
        added = True
    return pa, added


def _atmospheric(sep, pa, deltaR, parantel, variant):
    """:401-430 (3body :450-487): (sep_corrected, pa_angle, branch)."""
    pop = np.mean(pa) - parantel                         # :401
    if pop >= 90. and pop <= 270.:                       # :402
        deltasep = deltaR * np.cos(np.radians(180. - (pa - parantel)))      # :404
        sep_corrected = sep + deltasep
        if variant == 3:
            pa_mas = (sep_corrected) * (np.tan(np.radians(pa)))            # 3body :456
        else:
            pa_mas = (sep) * np.tan(np.radians(pa))                        # :407
        deltapa = deltaR * np.sin(np.radians(180. - (pa - parantel)))       # :408
        pa_mas_corrected = pa_mas + deltapa
        pa_angle = np.arctan(pa_mas_corrected / sep_corrected)             # :411
        if variant == 3:
            pa_angle = np.degrees(pa_angle)                                # 3body :461-462
            pa_angle[np.where(pa_angle < 0)] = pa_angle[np.where(pa_angle < 0)] + 180.
            branch = 5
        elif np.mean(pa) >= 90.:                                           # :412-415
            pa_angle = np.degrees(pa_angle) + 180.
            branch = 0
        else:
            pa_angle = np.degrees(pa_angle)
            branch = 1
    else:
        deltasep = deltaR * np.cos(np.radians(pa - parantel))              # :418
        sep_corrected = sep + deltasep
        if variant == 3:
            pa_mas = (sep_corrected) * np.tan(np.radians(pa))              # 3body :477
        else:
            pa_mas = (sep) * np.tan(np.radians(pa))                        # :421
        deltapa = deltaR * np.sin(np.radians(pa - parantel))               # :422
        pa_mas_corrected = pa_mas + deltapa
        second = (pop > 270) if variant == 2 else (np.mean(pa) > 270)      # :425 / 3body :481
        if pop > 270. and second:
            pa_angle = np.degrees(np.arctan(pa_mas_corrected / sep_corrected)) + 360.
            branch = 2
        elif pop > 270. and np.mean(pa) < 270:                             # :427
            pa_angle = np.degrees(np.arctan(pa_mas_corrected / sep_corrected)) + 180.
            branch = 3
        else:
            pa_angle = np.degrees(np.arctan(pa_mas_corrected / sep_corrected))
            branch = 4
    return sep_corrected, pa_angle, branch


def _pair(xs, ys, xc, yc, s, x_dist, y_dist, xdiff, ydiff, deltaR, variant):
    xs, ys, xc, yc = xs + 1, ys + 1, xc + 1, yc + 1      # :211-214
    xc_d, yc_d = _dedistort(xc, yc, x_dist, y_dist, xdiff, ydiff)
    xs_d, ys_d = _dedistort(xs, ys, x_dist, y_dist, xdiff, ydiff)
    deltay = yc_d - ys_d                                 # :255-256
    deltax = xc_d - xs_d
    rsquare = (deltay ** 2) + (deltax ** 2)              # :283
    r = np.sqrt(rsquare)
    sep = r * s["pixscale"]                              # :286
    pa, added = _pa(deltax, deltay, s, variant)
    mean_pa = np.mean(pa)
    sep_corrected, pa_angle, branch = _atmospheric(sep, pa, deltaR, s["parantel"], variant)
    out = {"sep_corrected": sep_corrected, "pa_angle": pa_angle, "branch_code": branch,
           "added_360": added, "pa_mean_uncorrected": float(mean_pa),
           "sep_median": np.median(sep_corrected), "sep_std": np.std(sep_corrected),   # :436
           "pa_median": np.median(pa_angle), "pa_std": np.std(pa_angle),             # :437
           "position_means": [np.mean(xs_d), np.mean(ys_d), np.mean(xc_d), np.mean(yc_d)]}
    if variant == 3:
        RA = sep_corrected * np.sin(np.radians(pa_angle))                 # 3body :508-512
        Dec = sep_corrected * np.cos(np.radians(pa_angle))
        out.update(ra=np.mean(RA), ra_std=np.std(RA), dec=np.mean(Dec), dec_std=np.std(Dec))
    else:
        RA = sep_corrected * np.cos(np.radians(pa_angle))                 # :446-450
        Dec = sep_corrected * np.sin(np.radians(pa_angle))
        out.update(ra=-np.mean(RA), ra_std=np.std(RA), dec=np.mean(Dec), dec_std=np.std(Dec))
    return out


def restate2(chains, scalars, x_dist=None, y_dist=None, xdiff=0, ydiff=0, deltaR=0.0):
    """apf_step3.py: one pair, the companion (columns 2, 3) about the star (0, 1)."""
    c = np.asarray(chains, dtype=np.float64)
    return [_pair(c[:, :, 0], c[:, :, 1], c[:, :, 2], c[:, :, 3], scalars, x_dist, y_dist,
                  xdiff, ydiff, deltaR, 2)]


def restate3(chains, scalars, x_dist=None, y_dist=None, xdiff=0, ydiff=0, deltaR=0.0):
    """3body/apf_step3_3body.py: b (columns 2, 3) and c (4, 5) about a (0, 1), :489-490."""
    c = np.asarray(chains, dtype=np.float64)
    return [_pair(c[:, :, 0], c[:, :, 1], c[:, :, k], c[:, :, k + 1], scalars, x_dist, y_dist,
                  xdiff, ydiff, deltaR, 3) for k in (2, 4)]


RESTATE = {2: restate2, 3: restate3}
