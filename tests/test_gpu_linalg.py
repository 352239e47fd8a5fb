"""GPU: the Jacobi eigh / SVD, Cholesky and triangular-inverse kernels of csrc/linalg_f64.hip against LAPACK on the spectra of tests/linalg_cases.py, at one or
more sizes per dispatch path; the refusals (indefinite, non-finite) and the A/B paths behind QEMB_JACOBI_*=0."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

import linalg_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(qlib):
    s = lc.LibSolver(qlib)
    s.name = "device"
    return s


@pytest.mark.parametrize("n", sorted(lc.EIGH_SIZES))
@pytest.mark.parametrize("family", lc.EIGH_FAMILIES)
def test_eigh_families(dev, family, n):
    lc.check_eigh(dev, family, n)


@pytest.mark.parametrize("scale_exp", [40, -40])
@pytest.mark.parametrize("n", lc.EIGH_SCALED_SIZES)
@pytest.mark.parametrize("family", lc.EIGH_FAMILIES)
def test_eigh_families_scaled(dev, family, n, scale_exp):
    lc.check_eigh(dev, family, n, scale_exp)


@pytest.mark.parametrize("n", lc.IN_BASIS_SIZES)
@pytest.mark.parametrize("family", lc.EIGH_FAMILIES)
def test_eigh_in_basis_families(dev, family, n):
    lc.check_eigh_in_basis(dev, family, n)


@pytest.mark.parametrize("shape", sorted(lc.SVD_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family", lc.SVD_FAMILIES)
def test_svd_families(dev, family, shape):
    lc.check_svd(dev, family, *shape)


@pytest.mark.parametrize("decades", lc.CHOL_DECADES)
@pytest.mark.parametrize("n", lc.CHOL_SIZES)
def test_cholesky_and_inverse_conditioned(dev, n, decades):
    A = lc.spd_matrix(n, decades)
    lc.check_cholesky(dev, A, f"kappa=1e{decades}")
    lc.check_tri_inverse(dev, A, f"kappa=1e{decades}")


def test_cholesky_and_inverse_octane_metric(dev):
    A = lc.octane_metric()
    lc.check_cholesky(dev, A, "octane12 metric")
    lc.check_tri_inverse(dev, A, "octane12 metric")


@pytest.mark.parametrize("index", range(4))
def test_cholesky_refusals(dev, index):
    label, A = lc.refusal_cases()[index]
    lc.check_cholesky_refuses(dev, A, label)


@pytest.mark.parametrize("place", lc.NONFINITE_PLACES)
@pytest.mark.parametrize("value", lc.NONFINITE_VALUES, ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("op,size", [("eigh", n) for n in lc.NONFINITE_EIGH_SIZES] + [("eigh_in_basis", 40)] + [("svd", s) for s in lc.NONFINITE_SVD_SHAPES]
                         + [("cholesky", n) for n in lc.NONFINITE_CHOL_SIZES], ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_nonfinite_input_is_refused(dev, op, size, value, place):
    lc.check_nonfinite(dev, op, size, value, place)


@pytest.mark.parametrize("setting", lc.AB_SETTINGS)
def test_ab_paths_in_a_fresh_process(qlib, setting):
    """QEMB_JACOBI_DB / _TWOSIDED / _BLOCK = 0 are read once per process: one fresh child per setting, one after another, through the same assertions."""
    env = dict(os.environ)
    for k in lc.AB_SETTINGS:
        env.pop(k, None)
    env[setting] = "0"
    r = subprocess.run([sys.executable, str(Path(lc.__file__).resolve())], env=env, cwd=str(Path(lc.__file__).resolve().parent.parent), timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"{setting}=0: exit {r.returncode}\n{r.stdout[-4000:]}"
    assert "ab child ok" in r.stdout
