"""Time the determinant-space FCI of solver="FCI-hip": one application of H split by kernel, and the whole fragment solve.

    python tools/fci_bench.py [out.jsonl]        (default profiles/fci_bench.jsonl; (n, nsocc) = (8,4), (10,5), (12,6), (14,7))

Per size one JSON line.  One application of H (qemb_op_fci_sigma_timed: device timers around the D gather, the product G = V D and the sigma gather; one untimed
application first, REPS timed ones: median, min, max): the product against the 78.6 TFLOP/s FP64 matrix peak with 2 n^4 N_det flops, each gather as an HBM pass
against 8 TB/s -- the D gather writes 8 n^2 N_det bytes twice (zeros, then the links) and reads c, the sigma gather reads D and the linked entries of G.  The
whole solve (DeviceFragment.solve_fci with energies, host clock around the call, which ends in a synchronisation): median of SOLVES warm calls, and the number
of applications of H it took."""
import ctypes as C
import json
import statistics
import sys
import time
from math import comb
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "oracle"))
from quemb_amd import _lib                                               # noqa: E402
from quemb_amd._lib import DeviceBuffer, check                            # noqa: E402
from quemb_amd.fragsolver import DeviceFragment                           # noqa: E402

FP64_MATRIX_PEAK, HBM_PEAK = 78.6e12, 8.0e12
SIZES = [(8, 4), (10, 5), (12, 6), (14, 7)]
REPS, SOLVES = 7, 3


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "fci_bench.jsonl"
    lib = _lib.init()
    rows = []
    for n, o in SIZES:
        ns = comb(n, o); N = ns * ns
        nlink = o * (n - o + 1)
        h, e1 = synthetic_fragment(n, o, 4000 + n)
        rng = np.random.default_rng(n)
        c = rng.standard_normal(N); c /= np.linalg.norm(c)
        dV, dc, ds = DeviceBuffer.from_numpy(e1.reshape(n * n, n * n)), DeviceBuffer.from_numpy(c), DeviceBuffer(N)
        ms = np.zeros((REPS, 3)); one = (C.c_double * 3)()
        for r in range(REPS):
            check(lib.qemb_op_fci_sigma_timed(n, o, h.ctypes.data, dV.ptr, dc.ptr, ds.ptr, one), "qemb_op_fci_sigma_timed", lib)
            ms[r] = list(one)
        for b in (dV, dc, ds):
            b.free()
        gather_bytes, sigma_bytes = 8.0 * N * (2 * n * n + 1), 8.0 * N * (n * n + 2 * nlink + 1)
        flops = 2.0 * n ** 4 * N
        med = np.median(ms, axis=0)
        fr = DeviceFragment(n, min(n, 4))
        fr.set_eri_s4(eri.pack_s4(e1))
        fr.set_energy_data(h, h, h, 1.0, [0])
        fr.solve_fci(o, h)
        walls, res = [], None
        for _ in range(SOLVES):
            t0 = time.perf_counter()
            res = fr.solve_fci(o, h)
            walls.append(1e3 * (time.perf_counter() - t0))
        fr.free()
        check(lib.qemb_trim(), "qemb_trim", lib)
        row = dict(n=n, nsocc=o, n_det=N, reps=REPS,
                   gather_ms=spread(ms[:, 0].tolist()), gemm_ms=spread(ms[:, 1].tolist()), sigma_gather_ms=spread(ms[:, 2].tolist()),
                   sigma_total_ms=float(med.sum()), gemm_tflops=flops / (med[1] * 1e9), gemm_frac_of_fp64_matrix_peak=flops / (med[1] * 1e-3) / FP64_MATRIX_PEAK,
                   gather_frac_of_hbm_peak=gather_bytes / (med[0] * 1e-3) / HBM_PEAK, sigma_gather_frac_of_hbm_peak=sigma_bytes / (med[2] * 1e-3) / HBM_PEAK,
                   solve_ms=spread(walls), solve_n_iter=res["n_iter"], solve_residual=res["residual"], e_corr_mo=res["e_corr_mo"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
