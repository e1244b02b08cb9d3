"""Best fit and Laplace approximation of a frame on MI355X (no counterpart in the reference,
which has no optimiser).

    python apf_map.py <dir>/N2.<date>.<frame>.LDIF.fits [--starts N] [--scatter X] [--seed S]
                      [--fixed-bkgd] [--fix NAME ...] [--max-steps K]

Writes ``map_fit.json`` and ``map_widths.json`` into the frame's results directory;
``apf_step2.py -i map [--start-scatter S] [--widths .../map_widths.json]`` starts from them.
See ``--help`` and olpefit_amd/mapcli.py.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from olpefit_amd.mapcli import main  # noqa: E402

if __name__ == "__main__":
    main(nsrc=2)
