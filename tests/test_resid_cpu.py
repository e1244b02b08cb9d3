"""Posterior model and residual images (olpe_resid_*, olpefit_amd/residuals.py): what needs
no GPU.

Argument validation of the C entries (OLPE_EINVAL with a message before any GPU call), the
host arithmetic of the mean / std planes from hand-made shifted sums (yardstick: np.mean /
np.std of the images the sums were made from), the .npz layout, and step 3 without
--residuals leaving exactly what it left before the option existed.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from olpefit_amd import _lib, pipeline, residuals, step3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _msg(lib):
    return lib.olpe_last_error().decode()


def test_null_handles_are_argument_errors(lib):
    h = C.c_void_p()
    d = np.zeros(64)
    p = d.ctypes.data_as(_lib._pd)
    n = C.c_longlong(0)
    assert lib.olpe_resid_create(None, None, C.byref(h)) == _lib.EINVAL and not h.value
    assert "NULL context" in _msg(lib)
    assert lib.olpe_resid_create(None, None, None) == _lib.EINVAL
    assert lib.olpe_resid_fold_ctx(None, None, 1, 1) == _lib.EINVAL
    assert lib.olpe_resid_fold_rows(None, p, 1) == _lib.EINVAL
    assert lib.olpe_resid_get(None, C.byref(n), C.byref(n), p, p, p, p) == _lib.EINVAL
    assert lib.olpe_resid_add(None, 1, 0, p, p, p, p) == _lib.EINVAL
    assert lib.olpe_resid_reset(None) == _lib.EINVAL
    assert lib.olpe_resid_finalize(None, p, p) == _lib.EINVAL
    lib.olpe_resid_destroy(None)                        # a no-op


def test_steps_and_counts_are_checked_before_the_handles_are_used(lib):
    """row_step / walker_step <= 0 and nsamples < 0 are refused before the object or the
    context is looked at (zeroed stand-ins here: no GPU call can have happened)."""
    fake_r, fake_c = C.create_string_buffer(4096), C.create_string_buffer(4096)
    r, c = C.cast(fake_r, C.c_void_p), C.cast(fake_c, C.c_void_p)
    for steps in ((0, 1), (1, 0), (-3, 2)):
        assert lib.olpe_resid_fold_ctx(r, c, *steps) == _lib.EINVAL
        assert "must be > 0" in _msg(lib)
    d = np.zeros(17)
    assert lib.olpe_resid_fold_rows(r, d.ctypes.data_as(_lib._pd), -1) == _lib.EINVAL
    assert "-1 samples" in _msg(lib)
    assert lib.olpe_resid_fold_rows(r, None, 5) == _lib.EINVAL
    assert lib.olpe_resid_finalize(r, None, None) == _lib.EINVAL
    assert lib.olpe_resid_add(r, 1, 0, None, None, None, None) == _lib.EINVAL


def test_signature_table_has_the_entries():
    for name in ("create", "destroy", "fold_ctx", "fold_rows", "get", "add", "reset", "finalize"):
        assert "olpe_resid_" + name in _lib.SIGNATURES
    assert len(residuals.PLANES) == 7 and len(residuals.SCALARS) == 8


def test_mean_std_from_shifted_sums_agree_with_numpy():
    """Shifted sums made by hand from a stack of images about a pivot image: mean_std
    returns np.mean / np.std (ddof 0) to rounding, where the unshifted one-pass formula
    would lose eight digits (values ~3e4 with scatter ~3)."""
    rng = np.random.RandomState(5)
    base = 3e4 * rng.uniform(0.1, 1.0, size=(9, 11))
    stack = base * (1.0 + 1e-4 * rng.normal(size=(301, 9, 11)))
    pivot = stack[0]
    s1 = (stack - pivot).sum(axis=0)
    s2 = ((stack - pivot) ** 2).sum(axis=0)
    mean, std = residuals.mean_std(pivot, s1, s2, stack.shape[0])
    ref = np.abs(stack).max()
    assert np.abs(mean - stack.mean(axis=0)).max() <= 1e-13 * ref
    assert np.abs(std - stack.std(axis=0)).max() <= 2e-13 * ref
    # one sample: its own image, no scatter
    mean, std = residuals.mean_std(pivot, np.zeros_like(pivot), np.zeros_like(pivot), 1)
    assert np.array_equal(mean, pivot) and not std.any()
    # rounding may leave the variance a hair below zero: clamped, not NaN
    _, std = residuals.mean_std(pivot, np.full_like(pivot, 3.0), np.full_like(pivot, 3.0 - 1e-15), 3)
    assert np.isfinite(std).all() and (std >= 0).all()


def test_npz_round_trip(tmp_path):
    """load_npz returns what np.savez wrote in Residuals.save's layout, NaN planes and
    the bool mask included."""
    rng = np.random.RandomState(2)
    planes = {k: rng.normal(size=(5, 5)) for k in residuals.PLANES}
    mask = np.zeros((5, 5), dtype=bool)
    mask[1, 2] = True
    for k in ("resid", "nresid", "mean_resid", "mean_nresid"):
        planes[k][mask] = np.nan
    path = str(tmp_path / "r.npz")
    with open(path, "wb") as f:
        np.savez(f, data=rng.normal(size=(5, 5)), mask=np.isnan(planes["nresid"]),
                 pivot=np.arange(17.0), best=np.arange(17.0) + 1, **planes,
                 scalar_samples=np.float64(12))
    z = residuals.load_npz(path)
    assert set(residuals.PLANES) <= set(z) and z["mask"].dtype == bool
    assert np.array_equal(z["mask"], mask) and float(z["scalar_samples"]) == 12.0
    for k in residuals.PLANES:
        assert np.array_equal(z[k], planes[k], equal_nan=True)
    assert np.array_equal(z["best"], np.arange(17.0) + 1)


def test_step3_without_residuals_is_unchanged(tmp_path, golden, capsys):
    """Without --residuals step 3 leaves the files, the summary keys and the printed lines
    it left before the option existed; --residuals with --from-moments is an argument
    error before anything is read."""
    g = golden("gr")
    chains = g["chains2"]
    N, M, ps = chains.shape
    image = str(tmp_path / "N2.20250127.00042.LDIF.fits")
    outdir = pipeline.image_paths(image)[2]
    os.makedirs(outdir)
    paths = [outdir + f"{w}_finalarray_mpi.csv" for w in range(M)]
    pipeline.write_chain_csvs(paths, chains.transpose(1, 0, 2), nan_row=True)
    before = set(os.listdir(outdir))
    capsys.readouterr()
    out = step3.main([image, "x", "-s", str(M)])
    lines = capsys.readouterr().out.splitlines()
    assert set(os.listdir(outdir)) == before | {"step3_summary.json"}
    assert list(out) == ["walkers", "rows_per_walker", "additional_burnin", "source",
                         "gr_rc_mean", "gr_rc_std", "parameters"]
    with open(outdir + "step3_summary.json", "rb") as f:
        assert f.read() == json.dumps(out, indent=1).encode()
    assert out["parameters"] == step3.summary(chains, nsrc=2)
    assert lines[0] == "Importing parameter arrays..." and len(lines) == 7 + 16
    assert not any("residual" in ln.lower() for ln in lines)
    for extra in (["--from-moments"], ["--residuals-thin", "0"]):
        with pytest.raises(SystemExit) as e:
            step3.main([image, "x", "-s", str(M), "-q", "--residuals"] + extra)
        assert e.value.code == 2
    assert set(os.listdir(outdir)) == before | {"step3_summary.json"}
