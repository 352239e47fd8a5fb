"""Time the DF mean field of the device -- one-electron integrals, J + K from the resident 3-index tensor, a whole RHF, BE on the shared tensor -- against the
routes that existed before it, in one process.

    python tools/dfjk_bench.py [out.jsonl]                 (default profiles/dfjk_bench.jsonl)

Cases: H8 / STO-3G, H8 / cc-pVDZ, octane / STO-3G (those of tools/jk_direct_bench.py).  Per case one JSON line; every time is the wall time around a synchronous
call, after two warm-up calls, as min / median / max of 9 repetitions (5 for the slow host contraction):
  one_electron_host_ms / one_electron_hip_ms   Mole.one_electron() against DeviceBasis.one_electron() on an uploaded basis
  df_jk_ms / cd_jk_ms         one warm J + K from the occupied orbitals (DFContext.get_jk_orbitals): etb auxiliaries / Cholesky factor at tol 1e-8;
                              df_fill_ms / cd_fill_ms the one-off fill of the context, *_bytes its resident tensor and the work space of a call
  df_j_ms, df_k_ms            the two halves alone
  direct_jk_ms                DeviceBasis.get_jk (integral-direct, pair stage cached)
  host_jk_packed_ms           the stored host contraction RHF._jk_packed of the 8-fold packed integrals
  rhf_*                       a whole RHF.kernel() on each route, the second (warm) of two runs: wall time, J / K builds, e_tot
  be2_*                       (H8 / STO-3G) BE2 one-shot MP2 on the DF mean field: BE filling its own context against reuse_mf_df=True, construction and solve"""
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


def timed(fn, reps=9, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(min=min(ts), median=statistics.median(ts), max=max(ts), reps=reps)


def once(fn):
    t = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t)


def core_orbitals(mol):
    S, T, V = mol.one_electron()
    w, U = np.linalg.eigh(S)
    X = U / np.sqrt(w) @ U.T
    _, c = np.linalg.eigh(X @ (T + V) @ X)
    return (X @ c)[:, : mol.nelectron // 2]


def rhf_run(mol, **kw):
    runs = []
    for _ in range(2):      # the second run is the warm one
        m = I.RHF(mol, **kw)
        calls = [0]
        jk0 = m._jk
        m._jk = lambda *a, _f=jk0, _c=calls: (_c.__setitem__(0, _c[0] + 1), _f(*a))[1]
        e, ms = once(m.kernel)
        runs.append(ms)
        m.free()
    return dict(ms_first=runs[0], ms_warm=runs[1], jk_builds=calls[0], e_tot=e, converged=bool(m.converged))


def be_rows(lib):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mol = next(iter(b4.cases()))[1]      # H8 / STO-3G: the chain the tracked fragmentation belongs to
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    mf = I.RHF(mol, integral_backend="hip", lib=lib, density_fit="etb")
    mf.kernel()
    out = {}
    for key, kw in (("be2_own_context", dict(auxbasis="etb")), ("be2_reuse_mf_df", dict(reuse_mf_df=True))):
        ts, e = [], None
        for _ in range(3):      # the last of three is quoted with the others
            t = time.perf_counter()
            be = BE(mf, fobj, lib=lib, distribute=False, int_transform="int-direct-DF-hip", integral_backend="hip", **kw)
            t1 = time.perf_counter()
            e = be.oneshot(solver="MP2")[0]
            ts.append((1e3 * (t1 - t), 1e3 * (time.perf_counter() - t1)))
        out[key] = dict(construct_ms=[a for a, _ in ts], oneshot_ms=[b for _, b in ts], e_corr=float(e))
    mf.free()
    return out


def main(out):
    from quemb_amd import _lib
    lib = _lib.init()
    rows = []
    cases = list(b4.cases())
    for name, mol in cases:
        N = mol.nao
        C0 = core_orbitals(mol)
        dm = 2.0 * C0 @ C0.T
        row = dict(case=name, nao=N, nshell=mol.nbas, natm=mol.natm, n_occ=C0.shape[1],
                   timing="wall time around synchronous calls, 2 warm-up calls, min / median / max in ms")
        # one-electron integrals
        basis = I.DeviceBasis(mol, lib)
        row["one_electron_host_ms"] = timed(mol.one_electron)
        row["one_electron_hip_ms"] = timed(basis.one_electron)
        h, d = mol.one_electron(), basis.one_electron()
        row["one_electron_max_rel_deviation"] = max(float(abs(a - b).max() / abs(b).max()) for a, b in zip(d, h))
        # J + K from the two kinds of resident tensor
        aux = I.make_auxmol(mol, "etb")
        for key, make in (("df", lambda: et.DFContext.from_mol(mol, aux, lib=lib)), ("cd", lambda: et.DFContext.from_cholesky(mol, tol=1e-8, lib=lib, basis=basis))):
            df, fill = once(make)
            row[f"{key}_naux"], row[f"{key}_fill_ms"] = int(df.naux), fill
            row[f"{key}_tensor_bytes"], row[f"{key}_jk_work_bytes"] = 8 * int(df.naux) * N * N, df.jk_bytes(C0.shape[1])
            row[f"{key}_jk_ms"] = timed(lambda: df.get_jk_orbitals(C0, 2.0))
            row[f"{key}_j_ms"] = timed(lambda: df.get_jk_orbitals(C0, 2.0, with_k=False))
            row[f"{key}_k_ms"] = timed(lambda: df.get_jk_orbitals(C0, 2.0, with_j=False))
            row[f"{key}_jk_eigh_ms"] = timed(lambda: df.get_jk(dm))      # the get_veff route: host eigh of the density first
            Jf, Kf = df.get_jk_orbitals(C0, 2.0)
            df.free()
            if key == "df":
                Jdf, Kdf = Jf, Kf
        row["direct_jk_ms"] = timed(lambda: basis.get_jk(dm))
        Jd, Kd = basis.get_jk(dm)
        row["cd_vs_direct_max_abs"] = max(float(abs(Jf - Jd).max()), float(abs(Kf - Kd).max()))
        row["df_vs_direct_max_abs"] = max(float(abs(Jdf - Jd).max()), float(abs(Kdf - Kd).max()))      # the fitting error of the etb auxiliaries
        eri8 = basis.eri(8)
        basis.free()
        mf = I.RHF(mol)
        mf._eri = eri8
        mf._jk_packed(dm)
        row["host_jk_packed_ms"] = timed(lambda: mf._jk_packed(dm), 5, warm=1)
        # a whole SCF on each route
        row["rhf_df"] = rhf_run(mol, integral_backend="hip", lib=lib, density_fit="etb")
        row["rhf_cholesky"] = rhf_run(mol, integral_backend="hip", lib=lib, density_fit=("cholesky", 1e-8))
        row["rhf_direct"] = rhf_run(mol, integral_backend="hip", lib=lib, direct=True)
        row["rhf_stored"] = rhf_run(mol, integral_backend="hip", lib=lib)
        if name == cases[0][0]:
            row.update(be_rows(lib))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out.write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    a = sys.argv[1:]
    main(Path(a[0]) if a else ROOT / "profiles" / "dfjk_bench.jsonl")
