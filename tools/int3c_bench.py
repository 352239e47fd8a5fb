"""Time the in-place fill of a DF context from the geometry (qemb_df_set_ints_from_basis: (P|Q), its factor and inverse, and (P|mu nu) by the device
integral kernels) against the host route (integrals.int2c2e + aux_e2 on the host, DFContext + set_ints upload) in the same process.

    python tools/int3c_bench.py [out.jsonl]                 (default profiles/int3c_bench.jsonl)
    python tools/int3c_bench.py --trace-case                 one device fill of the per-class case, to be run under `rocprofv3 --kernel-trace --stats`
    python tools/int3c_bench.py --per-class stats.csv [out.jsonl]     (default profiles/int3c_per_class.jsonl)

Cases: H8 / STO-3G, octane / STO-3G, H8 / cc-pVDZ, each with the even-tempered auxiliary basis.  Per case one JSON line: the best of three warm runs of
BOTH routes (each after a warm-up run of its own; wall time around the synchronous calls), the census of (shell pair, auxiliary shell) blocks per angular
class, and the time of writing the naux N^2 tensor once at 5.5 TB/s (what the tracked write passes reach, profiles/r05_kernel_roofline.jsonl).

--per-class: the case is an H16 chain with an s, s, p, d orbital basis and even-tempered auxiliaries up to g (every one of the 30 angular classes occurs,
~10^6 blocks).  From the kernel-stats CSV of a rocprofv3 run of --trace-case: per class the kernel time, the blocks, the bytes stored and the flops COUNTED
from the loops of int3c_core.h (not measured), and the ratio of the time to the write bound (5.5 TB/s) and to the vector FP64 bound (78.6 TFLOP/s)."""
import csv
import json
import re
import sys
import time
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from quemb_amd import integrals as I                                      # noqa: E402

HBM_WRITE = 5.5e12
FP64_VECTOR = 78.6e12


def cases():
    h8 = [["H", (0.0, 0.0, float(i))] for i in range(8)]
    yield "H8 / STO-3G", I.Mole(h8)
    yield "octane / STO-3G", I.Mole(ROOT / "tests" / "golden" / "octane.xyz")
    yield "H8 / cc-pVDZ", I.Mole(h8, basis="cc-pvdz")


def per_class_case():
    basis = {"H": I._CCPVDZ["H"] + [("d", [0.9, 0.35], [0.6, 0.5])]}
    mol = I.Mole([["H", (0.1 * (i % 2), 0.0, float(i))] for i in range(16)], basis=basis)
    return mol, I.make_auxmol(mol, "etb")


def census(mol, aux):
    lo = [s[1] for s in mol.shells]
    pairs = Counter((max(lo[i], lo[j]), min(lo[i], lo[j])) for i in range(len(lo)) for j in range(i + 1))
    la = Counter(s[1] for s in aux.shells)
    return {f"({a},{b}|{p})": n * m for (a, b), n in sorted(pairs.items()) for p, m in sorted(la.items())}


def best_of(fn, sync, reps=3):
    fn(); sync()                                                          # warm-up: code objects, pools, first-call costs
    best = 1e30
    for _ in range(reps):
        sync(); t = time.perf_counter()
        fn()
        sync(); best = min(best, time.perf_counter() - t)
    return best


def main_cases(out):
    from quemb_amd import _lib
    from quemb_amd import eri_transform as et
    lib = _lib.init()
    rows = []
    for name, mol in cases():
        aux = I.make_auxmol(mol, "etb")
        df = et.DFContext.empty(lib=lib)
        dev = best_of(lambda: df.set_ints_from_mol(mol, aux), lib.qemb_sync)
        df.free()
        keep = {}
        t2c = best_of(lambda: keep.__setitem__("j", I.int2c2e(aux)), lambda: None)
        t3c = best_of(lambda: keep.__setitem__("i", I.aux_e2(mol, aux)), lambda: None)

        def upload():
            dh = et.DFContext(j2c=keep["j"], lib=lib); dh.set_ints(keep["i"], mol.nao, "pqL"); lib.qemb_sync(); dh.free()
        tup = best_of(upload, lib.qemb_sync)
        host = t2c + t3c + tup
        nbytes = 8.0 * aux.nao * mol.nao * mol.nao
        row = dict(case=name, nao=mol.nao, naux=aux.nao, aux_lmax=max(s[1] for s in aux.shells), timing="best of 3 after a warm-up, both routes",
                   device_fill_ms=1e3 * dev, host_int2c2e_ms=1e3 * t2c, host_aux_e2_ms=1e3 * t3c, host_upload_and_factor_ms=1e3 * tup, host_route_ms=1e3 * host,
                   speedup=host / dev, tensor_bytes=nbytes, hbm_write_floor_ms=1e3 * nbytes / HBM_WRITE, device_over_floor=dev / (nbytes / HBM_WRITE),
                   blocks_per_class=census(mol, aux))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


def trace_case():
    from quemb_amd import _lib
    from quemb_amd import eri_transform as et
    lib = _lib.init()
    mol, aux = per_class_case()
    df = et.DFContext.empty(lib=lib)
    df.set_ints_from_mol(mol, aux)
    lib.qemb_sync()
    df.free()
    print(f"traced one fill: N = {mol.nao}, naux = {aux.nao}, {sum(census(mol, aux).values())} blocks")


def counted_flops(la, lb, lp):
    """flops of one primitive triple, counted from the loops of int3c_core.h (Boys series taken as 40 terms)"""
    nh = lambda L: (L + 1) * (L + 2) * (L + 3) // 6
    comps = lambda l: [(x, y, l - x - y) for x in range(l, -1, -1) for y in range(l - x, -1, -1)]
    L, LAB = la + lb + lp, la + lb
    r = 3 * sum(nh(L - n) - 1 for n in range(L + 1)) + 6 * 40
    g = sum(nh(LAB) * 4 * ((c[0] // 2 + 1) * (c[1] // 2 + 1) * (c[2] // 2 + 1)) for c in comps(lp))
    c = len(comps(lp)) * sum(3 * (a[0] + b[0] + 1) * (a[1] + b[1] + 1) * (a[2] + b[2] + 1) for a in comps(la) for b in comps(lb))
    e = 3 * 3 * 5 * (la + 1) * (lb + 1) * (LAB + 1)
    return r + g + c + e


def per_class(stats_csv, out):
    mol, aux = per_class_case()
    triples, blocks = Counter(), Counter()
    osh = [(s[1], len(s[2])) for s in mol.shells]
    ash = [(s[1], len(s[2])) for s in aux.shells]
    for i in range(len(osh)):
        for j in range(i + 1):
            (l1, n1), (l2, n2) = osh[i], osh[j]
            for lp, npr in ash:
                key = (max(l1, l2), min(l1, l2), lp)
                blocks[key] += 1; triples[key] += n1 * n2 * npr
    times = {}
    for r in csv.DictReader(open(stats_csv)):
        m = re.search(r"int3c_class_kernel<(\d), (\d), (\d)>", r["Name"])
        if m:
            key = tuple(int(x) for x in m.groups())
            times[key] = times.get(key, 0.0) + float(r["TotalDurationNs"])      # orbital fill and metric blocks of a class share the instantiation
    rows = []
    for key in sorted(blocks):
        la, lb, lp = key
        nbytes = 16.0 * (2 * la + 1) * (2 * lb + 1) * (2 * lp + 1) * blocks[key]
        flops = float(counted_flops(*key)) * triples[key]
        t = times.get(key)
        row = dict(cls="(%d,%d|%d)" % key, blocks=blocks[key], primitive_triples=triples[key], bytes_stored=nbytes, flops_counted=flops,
                   kernel_ms=None if t is None else t * 1e-6, note="kernel time includes the metric blocks of the same instantiation (l_b = 0 classes)" if lb == 0 else "")
        if t:
            row.update(time_over_write_bound=t * 1e-9 / (nbytes / HBM_WRITE), time_over_fp64_bound=t * 1e-9 / (flops / FP64_VECTOR))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--trace-case":
        trace_case()
    elif a and a[0] == "--per-class":
        per_class(a[1], Path(a[2]) if len(a) > 2 else ROOT / "profiles" / "int3c_per_class.jsonl")
    else:
        main_cases(Path(a[0]) if a else ROOT / "profiles" / "int3c_bench.jsonl")
