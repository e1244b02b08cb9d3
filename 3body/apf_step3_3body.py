"""LAPF 3-source step 3 front end (3body/apf_step3_3body.py's arguments, read of the
20-column chains and Gelman-Rubin statistics; with --astrometry also the separation /
position angle / RA / Dec of b and c about a, on the GPU, with --corner the corner
plot's histograms and quantile brackets, with --residuals the posterior's model and
residual images, with --autocorr the chains' autocorrelation times and effective sample
sizes, and with --photometry the companions' flux ratios and delta magnitudes, the FWHM and
the sources' S/N, and with --covariance the parameter covariance, the error ellipses of b
and c about a, the conditional widths and the multivariate Gelman-Rubin statistic, and with
--detect the companion detection map, its candidates and the contrast curve; see
olpefit_amd/step3.py).

    python 3body/apf_step3_3body.py <image> <system> -s <walkers> [-a <burn>]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from olpefit_amd.step3 import main  # noqa: E402

if __name__ == "__main__":
    main(nsrc=3)
