"""-m gpu: the k-point density-fitted route of the periodic driver on the device -- the three gfx950 passes of kdf_ops.hip against NumPy bit for bit, the
route against the supercell route (1e-10), the driver on build_chain(nk=3) against 'supercell-DF-hip' (1e-8 / 1e-8 / 5e-7, the tolerances of test_kbe_pbe.py),
the refusals and the determinism of the factor.  The checks are the ones tests/test_kdf_hostlogic.py runs on the scalar mock."""
import pytest

import test_kdf_hostlogic as th

pytestmark = pytest.mark.gpu


def test_backend_is_the_device(qlib):
    assert qlib.qemb_backend().decode() == "hip-gfx950"


def test_split_kernel_is_a_copy(qlib):
    th.check_split_kernel(qlib)


def test_stack_kernel_is_a_copy(qlib):
    th.check_stack_kernel(qlib)


def test_pack_kernel_is_one_multiplication(qlib):
    th.check_pack_kernel(qlib)


@pytest.mark.parametrize("kind", ["ring", "chain"])
def test_route_identity(qlib, kind):
    th.check_route_identity(qlib, kind)


def test_driver_kpoint_route_equals_supercell_route(qlib):
    th.check_driver(qlib)


def test_driver_with_the_block_resident(qlib):
    th.check_driver(qlib, matching=False, df_resident="block")


def test_refusals(qlib):
    th.check_refusals(qlib)


def test_determinism(qlib):
    th.check_determinism(qlib)
