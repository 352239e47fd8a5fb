"""Time the integral-direct J / K of the device (qemb_int_jk_direct) against the stored-integral mean field of the same process.

    python tools/jk_direct_bench.py [out.jsonl]                 (default profiles/jk_direct_bench.jsonl)
    python tools/jk_direct_bench.py --trace-case                 stored fill and direct J + K call of the per-class case, twice (the first round warms up),
                                                                 to be run under `rocprofv3 --kernel-trace --stats`
    python tools/jk_direct_bench.py --per-class kernel_trace.csv [out.jsonl]     (default profiles/jk_direct_per_class.jsonl)

Cases: H8 / STO-3G, H8 / cc-pVDZ, octane / STO-3G.  Per case one JSON line, every time the wall time around a synchronous call, after two warm-up calls,
as min / median / max of the repetitions:
  (a) direct_jk_ms      one J + K call with the pair stage and the Schwarz factors cached (what an SCF cycle costs); direct_first_ms: the first call on a
                        fresh basis (upload, pair stage, Schwarz launch included)
  (b) stored_fill_ms    the one-off qemb_int4c2e(sym = 8) fill copied to the host, and host_jk_packed_ms, the per-cycle contraction RHF._jk_packed does with
                        it (host_jk_unpack_ms: its first call, which unpacks the integrals to rows)
  (c) rhf_direct / rhf_stored   a whole RHF.kernel() both ways: wall time, cycles, e_tot
and direct_total_cheaper_for, the numbers n of J / K builds for which  first + (n - 1) direct  <  fill + unpack + n packed  (medians; "never": at no n <= 1000).
--trace-case / --per-class: the H8 chain with an s, s, p, d basis of tools/int4c_bench.py (all 21 classes).  From the kernel-trace CSV: per class the time of
the LAST dispatch of the stored-fill kernel (int4c_class_kernel: the warm second fill; the small Schwarz launches of the first direct call come before it) beside
that of the last dispatch of the digest kernel (int4c_jk_kernel: the warm second call), the canonical quartets, and the atomic adds the digest issues (nab + 1 + 2 (nsA + nsB) per item, 8 bytes each)."""
import csv
import json
import re
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np                                                        # noqa: E402
from quemb_amd import integrals as I                                      # noqa: E402
import int4c_bench as b4                                                  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(min=min(ts), median=statistics.median(ts), max=max(ts), reps=reps)


def density(mol):
    """a symmetric matrix of the size and scale of an RHF density (core guess): what the first cycle contracts"""
    S, T, V = mol.one_electron()
    w, U = np.linalg.eigh(S)
    X = U / np.sqrt(w) @ U.T
    _, c = np.linalg.eigh(X @ (T + V) @ X)
    Cm = X @ c
    no = mol.nelectron // 2
    return 2.0 * Cm[:, :no] @ Cm[:, :no].T


def main_cases(out):
    from quemb_amd import _lib
    lib = _lib.init()
    rows = []
    for name, mol in b4.cases():
        dm = density(mol)
        basis = I.DeviceBasis(mol, lib)
        t = time.perf_counter(); J, K = basis.get_jk(dm); first = 1e3 * (time.perf_counter() - t)      # includes the pair stage and the Schwarz launch
        direct = timed(lambda: basis.get_jk(dm), 9)
        fill = timed(lambda: basis.eri(8), 5)
        eri8 = basis.eri(8)
        need = basis.jk_bytes()
        basis.free()
        mf = I.RHF(mol)
        mf._eri = eri8
        t = time.perf_counter(); Jp, Kp = mf._jk_packed(dm); unpack = 1e3 * (time.perf_counter() - t)
        packed = timed(lambda: mf._jk_packed(dm), 5, warm=1)
        dev = max(float(abs(J - Jp).max() / abs(Jp).max()), float(abs(K - Kp).max() / abs(Kp).max()))
        scf = {}
        for key, kw in (("rhf_direct", dict(integral_backend="hip", lib=lib, direct=True)), ("rhf_stored", dict(integral_backend="hip", lib=lib))):
            runs = []
            for _ in range(2):      # the second run is the warm one
                m = I.RHF(mol, **kw)
                calls = [0]
                jk0 = m._jk
                m._jk = lambda d, _f=jk0, _c=calls: (_c.__setitem__(0, _c[0] + 1), _f(d))[1]
                t = time.perf_counter(); e = m.kernel(); runs.append(1e3 * (time.perf_counter() - t))
                if hasattr(m, "free"):
                    m.free()
            scf[key] = dict(ms_first=runs[0], ms_warm=runs[1], jk_builds=calls[0], e_tot=e, converged=bool(m.converged))
        # totals after n J / K builds: direct = first + (n - 1) d, stored = fill + unpack + n p
        d, p = direct["median"], packed["median"]
        ahead = [n for n in range(1, 1001) if first + (n - 1) * d < fill["median"] + unpack + n * p]
        if not ahead:
            verdict = "never (n <= 1000)"
        elif len(ahead) == 1000:
            verdict = "always (n <= 1000)"
        elif ahead[0] == 1:
            verdict = f"n <= {ahead[-1]}"       # cheaper per start, dearer per cycle: the stored route overtakes after that many builds
        else:
            verdict = f"n >= {ahead[0]}"
        row = dict(case=name, nao=mol.nao, nshell=mol.nbas, timing="wall time around synchronous calls, 2 warm-up calls, min / median / max in ms",
                   direct_jk_ms=direct, direct_first_ms=first, direct_device_bytes=need, stored_fill_ms=fill, stored_host_bytes=int(eri8.nbytes),
                   host_jk_unpack_ms=unpack, host_jk_packed_ms=packed, max_rel_deviation_direct_vs_stored=dev, direct_total_cheaper_for=verdict, **scf)
        print(json.dumps(row), flush=True)
        rows.append(row)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


def trace_case():
    from quemb_amd import _lib
    lib = _lib.init()
    mol = b4.per_class_case()
    npair = mol.nao * (mol.nao + 1) // 2
    buf = _lib.DeviceBuffer(npair * (npair + 1) // 2, lib=lib)
    b = I.DeviceBasis(mol, lib)
    dm = density(mol)
    for _ in range(2):      # the first round warms up (code objects, the cached pair stage); per_class reads the last dispatch of every kernel
        b.eri(8, out_dev=buf.ptr)
        lib.qemb_sync()
        b.get_jk(dm)
    b.free(); buf.free()
    print(f"traced two rounds of one stored fill and one direct J + K call: N = {mol.nao}, {sum(b4.census(mol)[0].values())} canonical shell quartets")


def per_class(trace_csv, out):
    mol = b4.per_class_case()
    q, pq = b4.census(mol)
    t_fill, t_jk = {}, {}
    for r in sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(r"int4c_(class|jk)_kernel<(\d), (\d), (\d), (\d)>", r["Kernel_Name"])
        if m:
            key = "(%s%s|%s%s)" % m.groups()[1:]
            d = t_fill if m.group(1) == "class" else t_jk
            d[key] = float(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))      # the last dispatch stays
    rows = []
    for key in sorted(q):
        la, lb, lc, ld = (int(c) for c in re.sub(r"\D", "", key))
        nsa, nsb, ncd = 2 * la + 1, 2 * lb + 1, (2 * lc + 1) * (2 * ld + 1)
        adds = q[key] * ncd * (nsa * nsb + 1 + 2 * (nsa + nsb))      # upper bound: filtered items and zero sums issue none
        f, j = t_fill.get(key), t_jk.get(key)
        row = dict(cls=key, timing="last of two dispatches, rocprofv3 kernel trace", shell_quartets=q[key], primitive_quartets_about=pq[key], stored_fill_kernel_ms=None if f is None else f * 1e-6,
                   digest_kernel_ms=None if j is None else j * 1e-6, atomic_adds_at_most=adds, atomic_bytes_at_most=8 * adds)
        if f and j:
            row["digest_over_fill"] = j / f
            row["atomic_gb_per_s_at_most"] = 8 * adds / j
        print(json.dumps(row), flush=True)
        rows.append(row)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--trace-case":
        trace_case()
    elif a and a[0] == "--per-class":
        per_class(a[1], Path(a[2]) if len(a) > 2 else ROOT / "profiles" / "jk_direct_per_class.jsonl")
    else:
        main_cases(Path(a[0]) if a else ROOT / "profiles" / "jk_direct_bench.jsonl")
