"""LAPF step 3 front end on MI355X output -- the reference apf_step3.py's arguments, chain
read, burn-in and Gelman-Rubin statistics; with --astrometry also its separation /
position-angle / RA / Dec summary, reduced on the GPU (the distortion tables, which the
reference does not ship, and deltaR are inputs; see olpefit_amd/step3.py); with --corner
the corner plot's 1-D / 2-D histograms and quantile brackets, counted on the GPU and written
to <frame>_corner.npz; with --residuals the posterior mean / scatter of the model and the
best sample's residual images, folded on the GPU and written to <frame>_residuals.npz and
four FITS files; with --autocorr an integrated autocorrelation time and effective sample size
per parameter, the lag sums folded on the GPU and written to <frame>_autocorr.npz; with
--photometry the companion's flux ratio and delta magnitude, the primary's flux, the FWHM and
the core fraction of every chain row, reduced on the GPU, and the reference's aperture S/N and
FWHM numbers, written to <frame>_photometry.npz and, with --astrometry, into the S/N and FWHM
fields of the epoch_grand_pasep line; with --covariance the parameter covariance and
correlations, the companion's error ellipse, the conditional widths and the multivariate
Gelman-Rubin statistic, the cross-column sums folded on the GPU and written to
<frame>_covariance.npz; with --detect the companion detection map (the matched filter of every
folded row's residual with its own PSF at every candidate position), its candidates and the
contrast curve, folded on the GPU and written to <frame>_detect.npz and three FITS files
(nothing is drawn).

    python apf_step3.py <dir>/N2.<date>.<frame>.LDIF.fits <system> -s <walkers> [-a <burn>]
        [--astrometry [--distortion X.fits Y.fits] [--delta-r MAS] [--prepost pre|post]]
        [--corner [--corner-bins N] [--corner-fine-bins N]]
        [--residuals [--residuals-thin N] [--bkgd-mode 0|1]]
        [--autocorr [--autocorr-max-lag N] [--autocorr-c X]]
        [--photometry [--photometry-thin N]]
        [--covariance [--covariance-thin N]]
        [--detect [--detect-thin N] [--detect-oversample 1|2|4] [--detect-threshold X]
                  [--detect-k K]]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from olpefit_amd.step3 import main  # noqa: E402

if __name__ == "__main__":
    main(nsrc=2)
