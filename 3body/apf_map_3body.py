"""Best fit and Laplace approximation, three-source variant, on MI355X (19 parameters;
``3body/apf_step2_3body.py -i map`` starts from the files it writes)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from olpefit_amd.mapcli import main  # noqa: E402

if __name__ == "__main__":
    main(nsrc=3)
