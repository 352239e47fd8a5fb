"""-m gpu: the perturbative triples correction E_(T) on the device -- the batched products of the particle term, the assembly kernel in its LDS and global
forms, the fixed-order sums, the fragment call and BE.ccsd_t -- the cases of tests/ccsd_t_cases.py, which tests/test_ccsd_t_hostlogic.py runs on the scalar
mock, against the twin of tests/ccsd_t_numpy.py.  Bars as stated there."""
import pytest

import ccsd_t_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("o,v", tc.op_shapes())
def test_op_against_the_twin(qlib, o, v):
    tc.check_op_against_twin(qlib, o, v)


@pytest.mark.parametrize("o,v,tile", tc.PIN_CASES + [tc.PRODUCTION_PIN])
def test_op_against_the_stored_twin(qlib, o, v, tile):
    """the configurations production runs, against the stored slab-wise twin (tests/golden/ccsd_t_pins.npz), bar 1e-10 of abs_sum: the default tile 16 with
    several tiles (M = ty o, N = tz o^2, K = v + o, batch tx, the shared B operand, ragged ldc), the assembly kernel at 1, 2, 3, 5, 8 and 14 waves, both
    forms of it around o = 20 | 21 with ragged tiles, and (20, 64, 8): the benchmark's n_occ with 120 tile triples.
    Measured |d| / abs_sum on the MI355X, in units of 1e-16 -- tile 16: (2, 35) 1.1, (5, 16) 0, (5, 17) 1.2, (5, 32) 1.8, (5, 33) 1.6, (5, 35) 1.2, (10, 35) 1.8;
    v = 5, tile 2: o = 8: 1.2, 9: 1.3, 11: 0, 13: 1.7, 16: 1.6, 19: 1.6; (20, 19, 8) 1.6, (21, 19, 8) 2.7, (21, 19, 4) 1.3 (the two tiles of (21, 19): 1.3 apart);
    (20, 64, 8) 3.4, the largest.  Each case under 0.2 s, (20, 64, 8) 0.7 s."""
    tc.check_op_against_pin(qlib, o, v, tile)


def test_empty_cases_and_bad_arguments(qlib):
    tc.check_empty_and_bad_arguments(qlib)


@pytest.mark.parametrize("residency", tc.RESIDENCIES)
@pytest.mark.parametrize("n,o", tc.FRAGMENTS)
def test_fragment(qlib, n, o, residency):
    tc.check_fragment(qlib, n, o, residency)


@pytest.mark.parametrize("n,o,residency", tc.CAP_FRAGMENTS)
def test_fragment_at_the_tile_caps(qlib, n, o, residency):
    """the automatic tile on both sides of o = 10 | 11 and o = 20 | 21, the second with the LDS | global form of the kernel, against the twin of the solve.
    Measured |d| on the MI355X (abs_sum 2e-3 .. 1e-2, bar 1e-8): (27, 10) 0, (30, 11) block 4e-19, factor 1.9e-17 (against the twin of the block solve),
    (40, 20) 0, (40, 21) 1.7e-18.  0.2 s each up to (30, 11); 2.7 s and 2.4 s at (40, 20) and (40, 21), the host twin's."""
    tc.check_cap_fragment(qlib, n, o, residency)


def test_fragment_at_bench_tiles_triples(qlib):
    """(T) of the stored n = 84, n_occ = 20 fragment (tests/test_gpu_fragment.py::test_fragment_at_bench_tiles) at production settings: the automatic tile
    is 8, 120 tile triples; e_t against the oracle's amplitudes through the slab-wise twin, stored once by tests/golden/make_golden_frag84_ccsd_t.py.
    Measured on the MI355X: |d| = 4.0e-15 at e_t = -5.80e-2 (bar 1e-8), 0.35 s."""
    import sys

    import numpy as np
    from helpers import GOLDEN, synthetic_fragment
    from qemb_oracle import eri
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    if str(GOLDEN) not in sys.path:
        sys.path.insert(0, str(GOLDEN))
    import make_golden_frag84 as mg
    g = np.load(GOLDEN / "frag84_ccsd_t.npz")
    n, o = int(g["n"]), int(g["o"])
    assert (n, o, int(g["seed"])) == (mg.N, mg.O, mg.SEED)
    h, e1 = synthetic_fragment(n, o, mg.SEED)
    fr = DeviceFragment(n, mg.NF)
    fr.set_eri_s4(eri.pack_s4(e1))
    del e1
    out = fr.solve(o, h, opts=default_opts(cc_conv_tol=1e-11, cc_conv_tol_normt=1e-9, scf_conv_tol=1e-12, scf_conv_tol_grad=1e-8), eeval=False)
    assert abs(out["e_corr_mo"] - float(g["e_corr"])) < tc.TOL
    got = fr.ccsd_t()
    err = abs(got["e_t"] - float(g["e_t"]))
    print(f"ccsd_t frag84: e_t = {got['e_t']:.12e} stored {float(g['e_t']):.12e} |d| = {err:.2e} (abs_sum {float(g['abs_sum']):.3e}) tile = {got['tile']} "
          f"triples = {got['n_tile_triples']} ms = {got['ms']}")
    assert got["tile"] == 8 and got["n_tile_triples"] == 120
    assert err < tc.TOL
    assert fr.ccsd_t()["e_t"] == got["e_t"]
    fr.free()


def test_solver_function_appends_it(qlib):
    tc.check_solver_function(qlib)


def test_refusals(qlib):
    tc.check_refusals(qlib)


def test_memory_guard(qlib):
    tc.check_memory_guard(qlib)


@pytest.mark.parametrize("which", ["h8", "octane"])
def test_be2_driver(qlib, which):
    tc.check_be(qlib, which)
