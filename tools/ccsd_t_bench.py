"""Time the perturbative triples correction E_(T) of a fragment that lives on its 3-index factor against the CCSD solve of the same fragment in the same process.

    python tools/ccsd_t_bench.py [out.jsonl] [--sizes 42,96,132,220] [--reps 3]        (default profiles/ccsd_t_bench.jsonl)

Sizes: the synthetic fragments n = 42 (o = 21), 96 (o = 9), 132 (o = 12) and the benchmark's n = 220 (o = 20), naux = 3 n.  Per size one JSON line, written as
soon as the size is done: wall time of a warm CCSD solve, then of DeviceFragment.ccsd_t (one warm-up call, the median of `reps` calls, every call listed) with
its split from the device timers of the call -- images, products, assembly -- and the host wall time of forming the integrals again; the counted flops
2 o^3 v^3 (o + v) of the expression, the flops of the products of the triples (K = v + o: the same count, from the tiles visited) and of every product of a
call, the integral transformation included (qemb_gemm_flop_count around one call); the products of the triples as a fraction of the FP64
matrix peak (78.6 TFLOP/s) beside the ring product's tracked 0.84; the bytes the six buffers of every tile triple are written and read with (8 o^3 v^3 each
way for the unique triples, counted from the tiles visited) over the assembly time; and the ratio of the call to the CCSD solve."""
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from quemb_amd import _lib                                               # noqa: E402
from quemb_amd.fragsolver import DeviceFragment, default_opts             # noqa: E402

FP64_MATRIX_PEAK = 78.6e12
RING_FRACTION = 0.84
SIZES = {42: (42, 21, 126), 96: (96, 9, 288), 132: (132, 12, 396), 220: (220, 20, 660)}


def factor_fragment(n, seed, naux, gap=2.0):
    rng = np.random.default_rng(seed)
    scale = 0.06 * min(1.0, (55.0 / n) ** 0.5)
    B = scale * rng.standard_normal((naux, n, n))
    B = 0.5 * (B + B.transpose(0, 2, 1))
    il = np.tril_indices(n)
    A = rng.standard_normal((n, n))
    return np.diag(gap * np.arange(n)) + 0.3 * 0.5 * (A + A.T), np.ascontiguousarray(B[:, il[0], il[1]])


def buffer_elements(o, v, tile):
    """doubles of the product buffers over all tile triples A >= B >= C (arrangements of equal tiles share a buffer)"""
    ext = [min(tile, v - t * tile) for t in range(-(-v // tile))]
    total = 0
    for a in range(len(ext)):
        for b in range(a + 1):
            for c in range(b + 1):
                if tile == 1 and a == c:
                    continue
                kinds = 1 if a == b == c else (3 if (a == b or b == c) else 6)
                total += kinds * ext[a] * ext[b] * ext[c] * o ** 3
    return total


def one_size(lib, n, o, naux, reps):
    v = n - o
    h, Bp = factor_fragment(n, 20260803, naux)
    fr = DeviceFragment(n, min(22, n // 2))
    fr.set_df_only(Bp)
    opts = default_opts()
    res = dict(n=n, o=o, v=v, naux=naux)
    out = fr.solve(o, h, opts=opts, eeval=False)                        # cold: allocations
    lib.qemb_sync(); t0 = time.perf_counter()
    out = fr.solve(o, h, opts=opts, eeval=False)
    lib.qemb_sync()
    res.update(ccsd_wall_ms=(time.perf_counter() - t0) * 1e3, ccsd_iterations=int(out["n_iter"]), e_ccsd=float(out["e_corr_mo"]), mo_route_factor=bool(fr.mo_route_used()[0]))
    flops = C.c_double()
    lib.qemb_gemm_flop_count(C.byref(flops), 1)
    r = fr.ccsd_t()                                                     # warm-up: allocations, code objects
    lib.qemb_gemm_flop_count(C.byref(flops), 1)
    calls = []
    for _ in range(reps):
        lib.qemb_sync(); t0 = time.perf_counter()
        r = fr.ccsd_t()
        lib.qemb_sync()
        calls.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, **r["ms"]))
    med = {k: statistics.median(c[k] for c in calls) for k in calls[0]}
    gemm_flops = flops.value                                            # every product of the warm-up call: the integral transformation and the triples
    nbuf = buffer_elements(o, v, r["tile"])
    triples_flops = 2.0 * nbuf * (v + o)
    res.update(e_t=r["e_t"], tile=r["tile"], n_tile_triples=r["n_tile_triples"], bytes=r["bytes"], t_wall_ms=med["wall_ms"], t_images_ms=med["images"], t_gemm_ms=med["gemm"],
               t_assemble_ms=med["assemble"], t_integrals_ms=med["integrals"], t_calls=calls, counted_flops=2.0 * o ** 3 * v ** 3 * (o + v), triples_gemm_flops=triples_flops,
               all_gemm_flops_of_a_call=gemm_flops, buffer_bytes_each_way=8.0 * nbuf,
               gemm_frac_of_fp64_matrix_peak=(triples_flops / (med["gemm"] * 1e-3) / FP64_MATRIX_PEAK) if med["gemm"] > 0 else None, ring_product_frac_tracked=RING_FRACTION,
               assemble_buffer_read_GBps=(8.0 * nbuf / (med["assemble"] * 1e-3) * 1e-9) if med["assemble"] > 0 else None,
               ratio_to_ccsd_solve=med["wall_ms"] / res["ccsd_wall_ms"])
    fr.free()
    return res


def main():
    args = [a for a in sys.argv[1:]]
    reps, sizes = 3, [42, 96, 132, 220]
    if "--reps" in args:
        k = args.index("--reps"); reps = int(args[k + 1]); del args[k:k + 2]
    if "--sizes" in args:
        k = args.index("--sizes"); sizes = [int(s) for s in args[k + 1].split(",")]; del args[k:k + 2]
    out = Path(args[0]) if args else ROOT / "profiles" / "ccsd_t_bench.jsonl"
    lib = _lib.init(0)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "a") as fh:
        for s in sizes:
            res = one_size(lib, *SIZES[s], reps)
            print(json.dumps({k: v for k, v in res.items() if k != "t_calls"}), flush=True)
            fh.write(json.dumps(res) + "\n"); fh.flush()


if __name__ == "__main__":
    main()
