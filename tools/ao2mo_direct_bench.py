"""Time the integral-direct AO -> fragment transform (qemb_ao2mo_direct) against the stored route of the same process.

    python tools/ao2mo_direct_bench.py [out.jsonl]                 (default profiles/ao2mo_direct_bench.jsonl)
    python tools/ao2mo_direct_bench.py --trace-case                 two direct transforms of the octane case (the first warms up), to be run under
                                                                    `rocprofv3 --kernel-trace --stats`: the stats split fill, pair-product and GEMM time

Cases: H8 / STO-3G, H8 / cc-pVDZ and octane / STO-3G with the embedding coefficients of their BE2 fragments.  Per case and tile size one JSON line, every time
the wall time around a synchronous call on a warm basis, two warm-up calls, min / median / max of 9 repetitions:
  direct_ms       one qemb_ao2mo_direct call for all fragments, coefficients up and blocks back to the host, as on the stored side
  stored_ms       qemb_aoeri_from_basis plus one qemb_ao2mo_dense per fragment
  *_device_bytes  qemb_ao2mo_direct_bytes; the stored route: 8 npair^2 for the resident integrals, the pair stage, and the two work arrays of ao2mo_dense for
                  the largest fragment
and the largest deviation of the two routes."""
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import numpy as np                                                        # noqa: E402
from quemb_amd import eri_transform as et                                 # noqa: E402
from quemb_amd import integrals as I                                      # noqa: E402
import int4c_bench as b4                                                  # noqa: E402

FRAGS = {"H8 / STO-3G": ("test_autogen_h_linear_be2", 1), "H8 / cc-pVDZ": ("test_autogen_h_linear_be2", 5), "octane / STO-3G": ("test_autogen_octane_be2", 1)}


def timed(fn, reps=9, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(min=min(ts), median=statistics.median(ts), max=max(ts), reps=reps)


def fragment_tas(name, mol, lib):
    """the embedding coefficients of the BE2 fragments (Schmidt decomposition of the converged mean field; the integrals of the fragments are not needed)"""
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    key, rep = FRAGS[name]
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", key)
    if rep > 1:
        fobj = fobj.replicate_sites(rep)
    mf = I.RHF(mol, integral_backend="hip", lib=lib, direct=True)
    mf.kernel()
    try:
        be = BE(mf, fobj, lib=lib, distribute=False, int_transform="int-direct-hip", integral_backend="hip", int_direct_tile=256)
    finally:
        mf.free()
    return [np.array(f.TA) for f in be.Fobjs]


def stored_bytes(basis, mol, ns):
    N, n = mol.nao, max(ns)
    npN, npn = N * (N + 1) // 2, n * (n + 1) // 2
    work = basis.jk_bytes() - 8 * (3 * N * N + mol.nbas ** 2) - 4096      # pair stage and lists (int4c_work_bytes)
    return 8 * npN * npN + work + 8 * (max(npN * N * N, n * n * npN) + max(n * npN * N, npn * N * N)) + 8 * npn * npn


def main_cases(out):
    from quemb_amd import _lib
    lib = _lib.init()
    rows = []
    for name, mol in b4.cases():
        tas = fragment_tas(name, mol, lib)
        ns = [t.shape[1] for t in tas]
        npair = mol.nao * (mol.nao + 1) // 2
        basis = I.DeviceBasis(mol, lib)

        def stored():
            ao = et.AOEri.from_basis(basis)
            try:
                return [ao.transform(t) for t in tas]
            finally:
                ao.free()

        ref = stored()
        t_stored = timed(stored)
        for tile in sorted({min(256, npair), npair}):
            got = basis.ao2mo(tas, tile_pairs=tile)
            dev = max(float(np.abs(g - r).max() / np.abs(r).max()) for g, r in zip(got, ref))
            t_direct = timed(lambda: basis.ao2mo(tas, tile_pairs=tile))
            row = dict(case=name, nao=mol.nao, npair=npair, n_frag=len(tas), n=ns, tile_pairs=tile, tiles=basis.tile_stats()[0],
                       timing="wall time around synchronous calls on a warm basis, 2 warm-up calls, min / median / max in ms", direct_ms=t_direct, stored_ms=t_stored,
                       direct_device_bytes=basis.ao2mo_bytes(ns, tile), stored_device_bytes=stored_bytes(basis, mol, ns), max_rel_deviation_direct_vs_stored=dev)
            print(json.dumps(row), flush=True)
            rows.append(row)
        basis.free()
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


def trace_case():
    from quemb_amd import _lib
    lib = _lib.init()
    name, mol = [c for c in b4.cases() if c[0].startswith("octane")][0]
    tas = fragment_tas(name, mol, lib)
    basis = I.DeviceBasis(mol, lib)
    for _ in range(2):
        basis.ao2mo(tas, tile_pairs=256)
    print(f"traced two direct transforms of {name}: {len(tas)} fragments, {basis.tile_stats()[0]} tiles of at most 256 AO pairs")
    basis.free()


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--trace-case":
        trace_case()
    else:
        main_cases(Path(a[0]) if a else ROOT / "profiles" / "ao2mo_direct_bench.jsonl")
