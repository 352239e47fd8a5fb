"""-m gpu: the one-pass ring preparation kernel (qemb_op_ccsd_ring_prep: R and W2 of the CCSD update from the raw ZB and ZC, the bases, the first ring
product and the two rank-n_occ corrections) and the rank-n_occ update of U with its transposed addend (qemb_op_ccsd_u_update) against the extended-precision
NumPy references at the shapes of tests/ring_prep_cases.py, and the CCSD solver with the rule forced on against forced off.

Bound of the op test, elementwise: |dev - ref| <= (o + 6) 2^-53 (|P1| + |W1base| + |ZB| + |W2base|/2 + |ZC|/2 + sum_l |t1 ovoo| terms) -- the a-priori bound
of a sum of that many terms in any order; it applies to the device result alone because the reference is accumulated and kept in np.longdouble."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import ring_prep_cases as cases

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("o,v", cases.SHAPES)
def test_ring_prep_matches_reference(qlib, o, v):
    """outputs within the a-priori bound, the NaN pads around both outputs untouched, ZB and ZC bit-unchanged, and a second call gives the same bits"""
    first = cases.run(qlib, o, v)
    cases.check_outputs(o, v, *first)
    again = cases.run(qlib, o, v)
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(first, again))


@pytest.mark.parametrize("o,v", cases.SHAPES)
def test_u_update_matches_reference(qlib, o, v):
    """the rank-n_occ update of U with its transposed addend: within (o + 2) 2^-53 sum |terms| of the extended-precision reference, NaN pads untouched, Z bit-unchanged,
    a second call gives the same bits"""
    first = cases.run_u(qlib, o, v)
    cases.check_u(o, v, *first)
    again = cases.run_u(qlib, o, v)
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(first, again))


def test_ring_prep_refuses_shapes_outside_the_rule(qlib):
    from quemb_amd._lib import DeviceBuffer
    o, v = cases.REFUSED
    b = DeviceBuffer(o * v * o * v)
    p = b.ptr
    assert qlib.qemb_op_ccsd_ring_prep(o, v, p, p, p, p, p, p, p, p, p, p) != 0      # the caller keeps the four passes
    assert qlib.qemb_op_ccsd_u_update(o, v, p, p, p, p) != 0
    assert qlib.qemb_op_ccsd_ring_prep_rule(o, v, 0) == 0


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from helpers import synthetic_scale
from quemb_amd import _lib
from quemb_amd.fragsolver import DeviceFragment, default_opts
n, o, nf, seed = 146, 16, 8, 14616
lib = _lib.init(0)
rng = np.random.default_rng(seed)
B = synthetic_scale(n) * rng.standard_normal((n, n, n))
B = 0.5 * (B + B.transpose(0, 2, 1))
il = np.tril_indices(n)
A = rng.standard_normal((n, n))
h = np.diag(2.0 * np.arange(n)) + 0.3 * 0.5 * (A + A.T)
fr = DeviceFragment(n, nf)
fr.set_df_only(np.ascontiguousarray(B[:, il[0], il[1]]))
out = fr.solve(o, h, opts=default_opts(), eeval=False)
print(json.dumps(dict(rule=int(lib.qemb_op_ccsd_ring_prep_rule(o, n - o, 0)), n_iter=int(out["n_iter"]), e_corr=float(out["e_corr_mo"]))))
"""


def test_solver_ring_prep_on_against_off():
    """One fragment just outside the replay regime, (o, v) = (16, 130): o^2 v^2 = 4 326 400 > 2^22 (v no multiple of the 16-wide tile), solved with
    QEMB_RING_PREP=0 and =1 in fresh child processes (side by side): the same iteration count and |dE_corr| <= 1e-11 Eh, an order below the solver's own
    1e-10 convergence threshold -- the two paths differ only in rounding order."""
    procs = {}
    for sw in ("0", "1"):
        env = dict(os.environ, QEMB_RING_PREP=sw)
        procs[sw] = subprocess.Popen([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    outs = {}
    for sw, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, (sw, p.returncode, se[-2000:])
        outs[sw] = json.loads(so.strip().splitlines()[-1])
    off, on = outs["0"], outs["1"]
    de = abs(on["e_corr"] - off["e_corr"])
    print(f"ring preparation on / off: n_iter {on['n_iter']} / {off['n_iter']}  E_corr {on['e_corr']:.12f}  |dE_corr| {de:.3e}")
    assert off["rule"] == 0 and on["rule"] == 1
    assert on["n_iter"] == off["n_iter"]
    assert de <= 1e-11


def test_solver_ring_prep_forced_in_the_replay_regime(qlib):
    """QEMB_RING_PREP=1 takes the pass in the replay regime too (the recorded update then contains the two kernels): one fragment of (o, v) = (6, 40), in one process
    (the switch is read at every solver set-up), forced on against forced off: the same iteration count, |dE_corr| <= 1e-11 Eh and the 1-RDM within the solver's
    conv_tol_normt = 1e-8"""
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    n, o, nf = 46, 6, 6
    h, e1 = synthetic_fragment(n, o, 4600 + o)
    s4 = eri.pack_s4(e1)
    outs = {}
    saved = os.environ.get("QEMB_RING_PREP")
    try:
        for sw in ("0", "1"):
            os.environ["QEMB_RING_PREP"] = sw
            assert qlib.qemb_op_ccsd_ring_prep_rule(o, n - o, 1) == int(sw)
            fr = DeviceFragment(n, nf)
            fr.set_eri_s4(s4)
            outs[sw] = fr.solve(o, h, opts=default_opts(), eeval=False)
    finally:
        if saved is None:
            os.environ.pop("QEMB_RING_PREP", None)
        else:
            os.environ["QEMB_RING_PREP"] = saved
    off, on = outs["0"], outs["1"]
    de = abs(on["e_corr_mo"] - off["e_corr_mo"])
    dr = float(np.abs(on["rdm1_emb"] - off["rdm1_emb"]).max())
    print(f"ring preparation forced on / off in the replay regime: n_iter {on['n_iter']} / {off['n_iter']}  |dE_corr| {de:.3e}  max |d rdm1| {dr:.3e}")
    assert on["n_iter"] == off["n_iter"]
    assert de <= 1e-11
    assert dr <= 1e-8
