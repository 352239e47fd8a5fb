"""Fixture for the -m gpu (T) test at the benchmark's n_occ = 20 (tests/test_gpu_ccsd_t.py::test_fragment_at_bench_tiles_triples): the fragment of
make_golden_frag84.py (n = 84, n_occ = 20, n_virt = 64) through the oracle's fragment RHF and RCCSD exactly as that script runs them, then the slab-wise
twin tests/ccsd_t_numpy.py::slabbed on the oracle's own t1, t2, MO integrals and orbital energies.  Stored: e_t and abs_sum (the scale of the sum), with
e_corr to tie the file to frag84.npz.  Several minutes of NumPy for the oracle and about four more for the twin on a handful of cores, hence stored.

    python tests/golden/make_golden_frag84_ccsd_t.py        (writes tests/golden/frag84_ccsd_t.npz)
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tests" / "golden"))
import ccsd_t_numpy as tn  # noqa: E402
import make_golden_frag84 as base  # noqa: E402
import mp2_numpy as mpn  # noqa: E402
from helpers import synthetic_fragment  # noqa: E402
from qemb_oracle import ccsd, scf  # noqa: E402


def main():
    t0 = time.time()
    N, O = base.N, base.O
    h, e1 = synthetic_fragment(N, O, base.SEED)
    mf = scf.rhf(h, e1, O, conv_tol=1e-12, conv_tol_grad=1e-8)
    assert mf["converged"]
    t1, t2, ecc, nit = ccsd.solve_ccsd(h, e1, O, mf["mo_coeff"], mf["mo_energy"], conv_tol=1e-11, conv_tol_normt=1e-9)
    print(f"RCCSD {ecc:.12f} in {nit} iterations ({time.time() - t0:.0f} s)", flush=True)
    stored = np.load(ROOT / "tests" / "golden" / "frag84.npz")
    assert abs(ecc - float(stored["e_corr"])) < 1e-12 and nit == int(stored["n_iter"])      # the solve frag84.npz holds
    mo = mpn.mo_eri(e1, mf["mo_coeff"])
    del e1
    blocks = tn.blocks(mo, O)
    del mo
    ref = tn.slabbed(t1.reshape(O, N - O), t2.reshape(O, O, N - O, N - O), *blocks, mf["mo_energy"][:O], mf["mo_energy"][O:])
    np.savez(ROOT / "tests" / "golden" / "frag84_ccsd_t.npz", n=N, o=O, seed=base.SEED, e_corr=ecc, e_t=ref["e_t"], abs_sum=ref["abs_sum"])
    print(f"frag84_ccsd_t: e_t = {ref['e_t']!r} abs_sum = {ref['abs_sum']!r} ({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
