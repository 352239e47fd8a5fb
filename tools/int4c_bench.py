"""Time the four-centre AO integrals on the device (qemb_int4c2e, 8-fold packed, left on the device) against the host source (Mole.eri_s1 plus packing to the
same form) in the same process.

    python tools/int4c_bench.py [out.jsonl]                 (default profiles/int4c_bench.jsonl)
    python tools/int4c_bench.py --trace-case                 one device fill of the per-class case, to be run under `rocprofv3 --kernel-trace --stats`
    python tools/int4c_bench.py --per-class stats.csv [out.jsonl]     (default profiles/int4c_per_class.jsonl)

Cases: H8 / STO-3G, H8 / cc-pVDZ, octane / STO-3G.  Per case one JSON line: the best of three warm runs of the device fill (after a warm-up; wall time around
the synchronous call), the best of two warm runs of the host route, and the census of canonical shell quartets per angular class.
--per-class: an H8 chain with an s, s, p, d basis (every one of the 21 classes occurs).  From the kernel-stats CSV of a rocprofv3 run of --trace-case: per
class the kernel time, the canonical shell quartets and the primitive quartets."""
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


def cases():
    h8 = [["H", (0.0, 0.0, float(i))] for i in range(8)]
    yield "H8 / STO-3G", I.Mole(h8)
    yield "H8 / cc-pVDZ", I.Mole(h8, basis="cc-pvdz")
    yield "octane / STO-3G", I.Mole(ROOT / "tests" / "golden" / "octane.xyz")


def per_class_case():
    basis = {"H": I._CCPVDZ["H"] + [("d", [0.9, 0.35], [0.6, 0.5])]}
    return I.Mole([["H", (0.1 * (i % 2), 0.0, float(i))] for i in range(8)], basis=basis)


def census(mol):
    """canonical shell quartets and primitive quartets per class (la lb|lc ld)"""
    pc = lambda a, b: a * (a + 1) // 2 + b
    pairs, prims = Counter(), Counter()
    sh = [(s[1], len(s[2])) for s in mol.shells]
    for i in range(len(sh)):
        for j in range(i + 1):
            key = (max(sh[i][0], sh[j][0]), min(sh[i][0], sh[j][0]))
            pairs[key] += 1; prims[key] += sh[i][1] * sh[j][1]
    q, pq = {}, {}
    for b in pairs:
        for k in pairs:
            if pc(*k) > pc(*b):
                continue
            name = "(%d%d|%d%d)" % (b + k)
            q[name] = pairs[b] * (pairs[b] + 1) // 2 if b == k else pairs[b] * pairs[k]
            pq[name] = prims[b] * prims[b] // 2 if b == k else prims[b] * prims[k]      # equal classes: about half of the square
    return q, pq


def best_of(fn, sync, reps=3):
    fn(); sync()
    best = 1e30
    for _ in range(reps):
        sync(); t = time.perf_counter()
        fn()
        sync(); best = min(best, time.perf_counter() - t)
    return best


def main_cases(out):
    from quemb_amd import _lib
    lib = _lib.init()
    rows = []
    for name, mol in cases():
        npair = mol.nao * (mol.nao + 1) // 2
        words = npair * (npair + 1) // 2
        buf = _lib.DeviceBuffer(words, lib=lib)
        b = I.DeviceBasis(mol, lib)
        dev = best_of(lambda: b.eri(8, out_dev=buf.ptr), lib.qemb_sync)
        got = buf.numpy()
        b.free(); buf.free()
        keep = {}
        t_s1 = best_of(lambda: keep.__setitem__("e", mol.eri_s1()), lambda: None, reps=2)
        t_pack = best_of(lambda: keep.__setitem__("p", I.pack_eri(keep["e"], 8)), lambda: None, reps=2)
        dev_rel = float(abs(got - keep["p"]).max() / abs(keep["p"]).max())
        q, pq = census(mol)
        row = dict(case=name, nao=mol.nao, nshell=mol.nbas, words_s8=words, timing="device: best of 3 after a warm-up; host: best of 2 after a warm-up",
                   device_fill_ms=1e3 * dev, host_eri_s1_ms=1e3 * t_s1, host_pack_ms=1e3 * t_pack, host_route_ms=1e3 * (t_s1 + t_pack),
                   speedup=(t_s1 + t_pack) / dev, max_rel_deviation=dev_rel, quartets_per_class=q)
        print(json.dumps(row), flush=True)
        rows.append(row)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


def trace_case():
    from quemb_amd import _lib
    lib = _lib.init()
    mol = per_class_case()
    npair = mol.nao * (mol.nao + 1) // 2
    buf = _lib.DeviceBuffer(npair * (npair + 1) // 2, lib=lib)
    b = I.DeviceBasis(mol, lib)
    b.eri(8, out_dev=buf.ptr)
    lib.qemb_sync()
    b.free(); buf.free()
    print(f"traced one fill: N = {mol.nao}, {sum(census(mol)[0].values())} canonical shell quartets")


def per_class(stats_csv, out):
    mol = per_class_case()
    q, pq = census(mol)
    times = {}
    for r in csv.DictReader(open(stats_csv)):
        m = re.search(r"int4c_class_kernel<(\d), (\d), (\d), (\d)>", r["Name"])
        if m:
            key = "(%s%s|%s%s)" % m.groups()
            times[key] = times.get(key, 0.0) + float(r["TotalDurationNs"])
        elif "int4c_pair_kernel" in r["Name"]:
            times["pair stage"] = times.get("pair stage", 0.0) + float(r["TotalDurationNs"])
    rows = []
    for key in sorted(q):
        t = times.get(key)
        row = dict(cls=key, shell_quartets=q[key], primitive_quartets_about=pq[key], kernel_ms=None if t is None else t * 1e-6)
        if t:
            row["ns_per_primitive_quartet"] = t / max(pq[key], 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    rows.append(dict(cls="pair stage (6 kernels)", kernel_ms=times.get("pair stage", 0.0) * 1e-6))
    print(json.dumps(rows[-1]), flush=True)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--trace-case":
        trace_case()
    elif a and a[0] == "--per-class":
        per_class(a[1], Path(a[2]) if len(a) > 2 else ROOT / "profiles" / "int4c_per_class.jsonl")
    else:
        main_cases(Path(a[0]) if a else ROOT / "profiles" / "int4c_bench.jsonl")
