"""The tail the CCSD, MP2 and FCI-hip fragment solvers share (Fragment::finish_solve: HF density, back-rotation of the 1-RDM, outputs, energies), as
tests/test_solve_tail_hostlogic.py (scalar mock device, CPU) and tests/test_gpu_solve_tail.py (MI355X) both run it: every function takes the library to drive.
Inputs are those of tests/fci_cases.py (helpers.synthetic_fragment_factor, tight SCF options, energy data on every fragment); every solve has a fresh fragment.
Shapes (n, nsocc): one occupied orbital, two generic ones, the largest the FCI solve takes in well under a second, and one without virtual orbitals."""
from functools import lru_cache

import numpy as np
import pytest

import fci_cases as fc

SHAPES = [(3, 1), (5, 2), (6, 3), (8, 3), (4, 4)]
PATHS = ("CCSD", "CCSD-relaxed", "MP2", "FCI-hip")
BATCH = [(5, 2), (8, 3)]
# |rdm1_emb - sym(C rdm1_mo C^T / 2)|: n <= 8, |C| <= 1, |dm| <= 2 bound the rounding of either evaluation by about 2 n^2 eps = 1.4e-14; 1e-12 leaves room
# for the summation orders of the t1 form, the device products and NumPy
BACKROT_TOL = 1e-12


@lru_cache(maxsize=None)
def solved(lib, n, o, path):
    """one solve of a fresh fragment with energies; computed once per library and left unchanged"""
    fr = fc.fragment(lib, n, o)
    try:
        return fr.solve_as("CCSD" if path == "CCSD-relaxed" else path, o, fc.inputs(n, o)[0], opts=fc.scf_opts(lib, relax_density=int(path == "CCSD-relaxed")), eeval=True)
    finally:
        fr.free()


def check_mean_field_part_is_shared(lib, n, o):
    """the four paths run the same fragment RHF and now the same code after it: what comes from the mean field alone is equal bit for bit"""
    ref = solved(lib, n, o, PATHS[0])
    for path in PATHS[1:]:
        out = solved(lib, n, o, path)
        for k in ("mo_coeff", "mo_energy", "e_scf", "ebe_hf", "scf_cycles"):
            assert np.array_equal(np.asarray(out[k]), np.asarray(ref[k])), (path, k)


def check_back_rotation(lib, n, o, path):
    out = solved(lib, n, o, path)
    D, C = out["rdm1_emb"], out["mo_coeff"]
    assert np.array_equal(D, D.T)
    R = 0.5 * C @ out["rdm1_mo"] @ C.T
    err = np.abs(D - 0.5 * (R + R.T)).max()
    print(f"back-rotation ({n},{o}) {path}: max |rdm1_emb - sym(C rdm1_mo C^T / 2)| = {err:.2e}")
    assert err <= BACKROT_TOL
    if o == n:      # no virtual orbitals: the mean-field results
        assert out["e_corr_mo"] == 0.0 and out["n_iter"] == 0 and out["lambda_iters"] == 0
        assert np.array_equal(out["rdm1_mo"], 2.0 * np.eye(n)) and out["e_frag"][1] == 0.0


def check_energy_data_is_required(lib, solver):
    """eeval on a fragment that never received set_energy_data: refused with QEMB_ERR_ARG by every solver"""
    from quemb_amd import _lib
    from quemb_amd.fragsolver import DeviceFragment
    from qemb_oracle import eri
    n, o = 5, 2
    h, e1 = fc.inputs(n, o)[:2]
    fr = DeviceFragment(n, fc.sites(n)[0], lib=lib)
    try:
        fr.set_eri_s4(eri.pack_s4(e1))
        with pytest.raises(_lib.QembError, match=r"set_energy_data\(h1, veff0, \.\.\.\) before an energy evaluation") as ei:
            fr.solve_as(solver, o, h, opts=fc.scf_opts(lib), eeval=True)
        assert ei.value.status == _lib.QEMB_ERR_ARG
        assert fr.solve_as(solver, o, h, opts=fc.scf_opts(lib), eeval=False)["e_scf"] == solved(lib, n, o, solver)["e_scf"]      # (and the fragment stays usable)
    finally:
        fr.free()


def check_batch_equals_serial(lib, solver):
    """solve_batch of two fragments of different sizes: the dicts of the one-by-one solves, bit for bit"""
    from quemb_amd.fragsolver import solve_batch
    frs = [fc.fragment(lib, n, o) for n, o in BATCH]
    try:
        outs = solve_batch(frs, [o for _, o in BATCH], [fc.inputs(n, o)[0] for n, o in BATCH], opts=fc.scf_opts(lib), eeval=True, solver=solver)
    finally:
        for fr in frs:
            fr.free()
    for (n, o), out in zip(BATCH, outs):
        ref = solved(lib, n, o, solver)
        assert set(out) == set(ref)
        for k, x in ref.items():
            assert (out[k] is None) if x is None else np.array_equal(np.asarray(out[k]), np.asarray(x)), (n, o, k)
