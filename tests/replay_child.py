"""The body of a child process of test_gpu_fragment.py::test_graph_replay_equals_eager_in_fresh_processes (QEMB_GRAPH is read once per process: the environment
already holds the setting).  One lone fragment of n = 12, n_occ = 4 -- the first Hamiltonian of check_solve_batch_equals_one_by_one -- is solved twice, with the
default DIIS space and with cc_diis_space = 1 (no extrapolation: the update then writes to another place), and what came out goes into the .npz named on the
command line."""
import os
import sys

import numpy as np

N, O, NF, SEED = 12, 4, 4, 900
KEYS = ("n_iter", "e_corr_mo", "t1", "t2", "rdm1_emb")
CASES = {"diis_default": {}, "diis_1": {"cc_diis_space": 1}}


def run_child(path):
    from quemb_amd import _lib
    from quemb_amd.fragsolver import DeviceFragment, default_opts
    from qemb_oracle import eri
    from test_hostlogic_fragment import _problem
    lib = _lib.init(int(os.environ.get("LOCAL_RANK", "0")))
    h, e1 = _problem(N, O, NF, SEED)[:2]
    out = {}
    for case, kw in CASES.items():
        fr = DeviceFragment(N, NF, lib=lib)
        fr.set_eri_s4(eri.pack_s4(e1))
        res = fr.solve(O, h, opts=default_opts(lib, **kw), eeval=False, want_t2=True)
        for k in KEYS:
            out[f"{case}.{k}"] = np.asarray(res[k])
        fr.free()
    np.savez(path, **out)
    print("replay child ok: QEMB_GRAPH =", os.environ.get("QEMB_GRAPH"))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, ".."), os.path.join(here, "..", "oracle")]
    run_child(sys.argv[1])
