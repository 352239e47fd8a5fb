"""Time the determinant-space FCI of solver="FCI-hip": one application of H split by kernel, and the whole fragment solve.

    python tools/fci_bench.py [out.jsonl]        (default profiles/fci_bench.jsonl; (n, nsocc) = (8,4), (10,5), (12,6), (14,7))

Per size one JSON line.  One application of H (qemb_op_fci_sigma_timed: device timers around the D gather, the product G = V D and the sigma gather; one untimed
application first, REPS timed ones: median, min, max): the product against the 78.6 TFLOP/s FP64 matrix peak with 2 n^4 N_det flops, each gather as an HBM pass
against 8 TB/s -- the D gather writes 8 n^2 N_det bytes twice (zeros, then the links) and reads c, the sigma gather reads D and the linked entries of G.  The
whole solve (DeviceFragment.solve_fci with energies, host clock around the call, which ends in a synchronisation): median of SOLVES warm calls, and the number
of applications of H it took.

    python tools/fci_bench.py --size N,NSOCC --slab-rows R --mem-limit-gb L [out.jsonl]

One size in slabs (DeviceFragment.set_fci_slab: R = 0 off, k > 0 rows, -1 automatic) under an explicit memory limit for the solve and for the 2-RDM; the row is
APPENDED to the file.  Meant for one run per process: the solve once, cold (host clock), then the 2-RDM, then one application of H at the slab height the solve
used with its three steps timed and summed over the slabs (qemb_op_fci_sigma_slab; unslabbed: qemb_op_fci_sigma_timed).  There is no independent reference at
n = 15, 16: such a row is written only if Tr dm1 = 2 nsocc to 1e-10, sum h dm1 + 1/2 sum (pq|rs) dm2 = e_fci to 1e-8 and the residual is at most conv_tol.  Every
row records the three figures and whether they hold (`checks_hold`), and below 12 M determinants | |c|^2 - 1 | of the returned vector."""
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


def slab_row(lib, n, o, slab_rows, limit_gb):
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    from quemb_amd.fragsolver import default_fci_opts
    ns = comb(n, o); N = ns * ns
    h, e1 = synthetic_fragment(n, o, 4000 + n)
    limit = int(limit_gb * 1e9)
    fo = default_fci_opts(lib)
    fr = DeviceFragment(n, min(n, 4))
    fr.set_eri_s4(eri.pack_s4(e1))
    fr.set_energy_data(h, h, h, 1.0, [0])
    fr.set_fci_mem_limit(limit); fr.set_rdm2_mem_limit(limit)
    fr.set_fci_slab(slab_rows)
    t0 = time.perf_counter()
    res = fr.solve_fci(o, h, fci_opts=fo, want_civec=N <= 12_000_000)      # (the vector comes back where it is small: its norm is recorded with the row)
    solve_ms = 1e3 * (time.perf_counter() - t0)
    rows_used, n_slab = fr.fci_slab_used()
    t0 = time.perf_counter()
    dm2 = fr.make_rdm2("FCI-hip", with_dm1=True)
    rdm2_ms = 1e3 * (time.perf_counter() - t0)
    rdm2_rows, rdm2_slabs = fr.fci_slab_used()
    fr.free()
    check(lib.qemb_trim(), "qemb_trim", lib)
    Cm, dm1 = res["mo_coeff"], res["rdm1_mo"]
    hmo = Cm.T @ h @ Cm
    Vmo = np.einsum("ijkl,ip,jq,kr,ls->pqrs", e1, Cm, Cm, Cm, Cm, optimize=True)
    trace_err = abs(float(np.trace(dm1)) - 2 * o)
    e_rdm_err = abs(float(np.einsum("pq,pq->", hmo, dm1) + 0.5 * np.einsum("pqrs,pqrs->", Vmo, dm2)) - res["e_fci"])
    norm_err = None if res["civec"] is None else abs(float(np.sum(res["civec"] ** 2)) - 1.0)
    ok = trace_err <= 1e-10 and e_rdm_err <= 1e-8 and res["residual"] <= fo.conv_tol
    c = np.random.default_rng(n).standard_normal(N); c /= np.linalg.norm(c)
    dV, dc, ds = DeviceBuffer.from_numpy(e1.reshape(n * n, n * n)), DeviceBuffer.from_numpy(c), DeviceBuffer(N)
    one = (C.c_double * 3)()
    if rows_used > 0:
        check(lib.qemb_op_fci_sigma_slab(n, o, h.ctypes.data, dV.ptr, dc.ptr, ds.ptr, rows_used, one), "qemb_op_fci_sigma_slab", lib)
    else:
        check(lib.qemb_op_fci_sigma_timed(n, o, h.ctypes.data, dV.ptr, dc.ptr, ds.ptr, one), "qemb_op_fci_sigma_timed", lib)
    for b in (dV, dc, ds):
        b.free()
    flops = 2.0 * n ** 4 * N
    row = dict(n=n, nsocc=o, n_det=N, slab_rows=slab_rows, mem_limit_gb=limit_gb, rows_used=rows_used, n_slab=n_slab, rdm2_rows_used=rdm2_rows, rdm2_n_slab=rdm2_slabs,
               gather_ms=one[0], gemm_ms=one[1], sigma_gather_ms=one[2], sigma_total_ms=float(sum(one)), gemm_tflops=flops / (one[1] * 1e9),
               solve_ms=solve_ms, solve_n_iter=res["n_iter"], solve_residual=res["residual"], e_fci=res["e_fci"], e_corr_mo=res["e_corr_mo"], rdm2_ms=rdm2_ms,
               norm_err=norm_err, trace_err=trace_err, e_from_rdms_err=e_rdm_err, checks_hold=bool(ok))
    print(json.dumps(row), flush=True)
    return row if ok or n < 15 else None


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--size", default=None, help="N,NSOCC")
    ap.add_argument("--slab-rows", type=int, default=None, help="0 off, k > 0 alpha rows per slab, -1 automatic")
    ap.add_argument("--mem-limit-gb", type=float, default=None)
    args = ap.parse_args()
    if args.slab_rows is not None:
        if args.size is None or args.mem_limit_gb is None:
            ap.error("--slab-rows goes with --size N,NSOCC and --mem-limit-gb L")
        n, o = (int(x) for x in args.size.split(","))
        out = Path(args.out) if args.out else ROOT / "profiles" / "fci_bench.jsonl"
        row = slab_row(_lib.init(), n, o, args.slab_rows, args.mem_limit_gb)
        if row is None:
            print("fci_bench: the checks of the row do not hold; nothing written", file=sys.stderr)
            sys.exit(3)
        out.parent.mkdir(parents=True, exist_ok=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        return
    from helpers import synthetic_fragment
    from qemb_oracle import eri
    out = Path(args.out) if args.out else ROOT / "profiles" / "fci_bench.jsonl"
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
    kept = [ln for ln in out.read_text().splitlines() if '"slab_rows"' in ln] if out.exists() else []      # the rows of the slab mode stay
    out.write_text("".join(json.dumps(r) + "\n" for r in rows) + "".join(ln + "\n" for ln in kept))


if __name__ == "__main__":
    main()
