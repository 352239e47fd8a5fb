"""Measure the orbital localisation on the device (quemb_amd.lo, csrc/loc_ops.hip) against its NumPy twin, and what localising the bath does to the semi-sparse screen.

    python tools/loc_bench.py [out.jsonl]        (default profiles/loc_bench.jsonl; needs a GPU)

Systems: octane (tests/golden/octane.xyz) and all-trans hexadecane C16H34 built here, both in the built-in STO-3G basis, mean field from integral-direct J / K on
the device.  One JSON line per (system, target, method):
  target "occupied"  the occupied canonical orbitals (m = n_occ): Boys, PM (lowdin populations), ER (on the Cholesky factor of the AO integrals, tol 1e-8: K = its rank), cholesky
  target "bath"      the bath columns TA[:, n_f:] of the fragments made of three neighbouring carbons and their hydrogens (Schmidt decomposition as BE does it), all
                     fragments of the chain one after the other: Boys, PM, ER, cholesky
Per line: K, m (bath: the largest), the variant, the sweep count (bath: summed), the wall time of the device call with its transfers (best of 3) and of the NumPy twin
(tests/loc_numpy.py, once), f before and after; for the bath the number of (mu, i) pairs that get_AO_per_MO keeps, |S_abs TA|(mu, i) >= 1e-5 (the sparse route's
default MO_coeff_epsilon), over the bath columns (the twin is not run for ER on the baths: with K = naux it takes minutes per system; its occupied-orbital rows have it) of all fragments before and after the localisation.  Nothing is tuned: what comes out is written."""
import ctypes as C
import json
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import loc_numpy as twin                                                  # noqa: E402
from quemb_amd import _lib, integrals, lo                                 # noqa: E402
from quemb_amd import eri_sparse_DF as sdf                                # noqa: E402
from quemb_amd import eri_transform as et                                 # noqa: E402
from quemb_amd.integrals import RHF, Mole                                 # noqa: E402

EPS = 1e-5


def alkane(n):
    """all-trans C_n H_2n+2: C-C 1.54 A, C-H 1.09 A, tetrahedral angles; the carbons zig-zag in the xy plane"""
    t = np.deg2rad(109.4712206) / 2.0
    dx, dy = 1.54 * np.sin(t), 1.54 * np.cos(t)
    hx, hz = 1.09 * np.cos(t), 1.09 * np.sin(t)
    atoms = []
    for i in range(n):
        s = 1.0 if i % 2 == 0 else -1.0
        c = np.array([i * dx, s * dy / 2.0, 0.0])
        atoms.append(("C", tuple(c)))
        atoms.append(("H", tuple(c + [0.0, s * hx, hz])))
        atoms.append(("H", tuple(c + [0.0, s * hx, -hz])))
        if i in (0, n - 1):      # the third hydrogen of a methyl group continues the zig-zag
            e = -1.0 if i == 0 else 1.0
            atoms.append(("H", tuple(c + [e * 1.09 * np.sin(t), -s * 1.09 * np.cos(t), 0.0])))
    return atoms


def carbon_fragments(mol):
    """AO lists of every three neighbouring carbons with their hydrogens"""
    carbons = [i for i, a in enumerate(mol.atom) if a[0] == "C"]
    owner = {}
    for i, a in enumerate(mol.atom):
        if a[0] == "H":
            owner[i] = min(carbons, key=lambda c: np.linalg.norm(np.asarray(mol.atom[c][1]) - np.asarray(a[1])))
    ao_atom = np.asarray(mol.ao_atom)
    frags = []
    for k in range(len(carbons) - 2):
        trio = carbons[k:k + 3]
        atoms = set(trio) | {h for h, c in owner.items() if c in trio}
        frags.append([int(x) for x in np.nonzero(np.isin(ao_atom, sorted(atoms)))[0]])
    return frags


def timed_get_loc(lib, mol, C0, method, reps=3, df=None, cache=None):
    best, st, out = None, {}, None
    for _ in range(reps):
        st = {}
        lib.qemb_sync(); t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out = lo.get_loc(mol, C0, method, lib=lib, stats=st, df=df, cache=cache)
        lib.qemb_sync(); ms = 1e3 * (time.perf_counter() - t0)
        best = ms if best is None else min(best, ms)
    return out, st, best


def stack_of(lib, mol, S, C0, method, tensor=None):
    if method == "ER":      # the 3-index factor of the columns, formed on the host for the twin (the device forms its own and keeps it there)
        return np.einsum("mi,Pmn,nj->Pij", C0, tensor, C0, optimize=True)
    if method == "boys":
        return np.array([C0.T @ x @ C0 for x in integrals.dipole(mol, backend="hip", lib=lib)])
    return lo.population_stack(mol, C0, S, "lowdin")


def device_and_twin(lib, mol, S, C0, method, df=None, tensor=None, with_twin=True, cache=None):
    """-> (C_loc, row): the device call through get_loc, the sweeps alone (joint_diag on the finished stack) and the NumPy twin on the same stack"""
    Cl, st, ms = timed_get_loc(lib, mol, C0, method, df=df, cache=cache)
    row = dict(method=method, get_loc_ms=ms)
    if method == "cholesky":
        return Cl, row
    Q = stack_of(lib, mol, S, C0, method, tensor)
    best = None
    for _ in range(3):
        lib.qemb_sync(); t0 = time.perf_counter()
        lo.joint_diag(Q, lib=lib)
        lib.qemb_sync(); d = 1e3 * (time.perf_counter() - t0)
        best = d if best is None else min(best, d)
    row.update(K=st["K"], m=st["m"], in_lds=st["in_lds"], sweeps=st["sweeps"], converged=st["converged"], f_before=st["f_before"], f_after=st["f_after"], joint_diag_ms=best)
    if with_twin:
        t0 = time.perf_counter()
        _, _, sw_t, f_t, cv_t = twin.joint_diag(Q)
        row.update(twin_ms=1e3 * (time.perf_counter() - t0), twin_sweeps=sw_t, twin_f=f_t, twin_converged=bool(cv_t))
    return Cl, row


def one_system(lib, name, mol):
    rows = []
    mf = RHF(mol, integral_backend="hip", lib=lib, direct=True)
    mf.kernel()
    S = np.asarray(mf.get_ovlp())
    nocc = mol.nelectron // 2
    Cocc = np.array(mf.mo_coeff)[:, :nocc]
    df = et.DFContext.from_cholesky(mol, tol=1e-8, lib=lib)
    tensor, ident = np.empty((df.naux, mol.nao, mol.nao)), C.c_int()
    _lib.check(lib.qemb_op_df_get_ints(df.h, tensor.ctypes.data, C.byref(ident)), "qemb_op_df_get_ints", lib)
    for method in ("boys", "PM", "ER", "cholesky"):
        _, row = device_and_twin(lib, mol, S, Cocc, method, df=df, tensor=tensor)
        rows.append(dict(system=name, nao=mol.nao, target="occupied", **row))
        print(json.dumps(rows[-1]), flush=True)
    w, v = np.linalg.eigh(S)
    W = (v / np.sqrt(w)) @ v.T
    lmo = W.T @ S @ np.array(mf.mo_coeff)
    S_abs = sdf.approx_S_abs(mol, lib=lib)
    baths, cache = [], {}      # cache: the dipole integrals and S^1/2 of the molecule, formed once for all baths as BE does
    for ao in carbon_fragments(mol):
        TA_lo, n_f, n_b = et.schmidt_decomposition(lmo, nocc, ao, thr_bath=1e-10, lib=lib, method="subspace")
        baths.append((W @ TA_lo)[:, n_f:])
    kept = lambda Bs: int(sum((np.abs(S_abs @ B) >= EPS).sum() for B in Bs))
    for method in ("boys", "PM", "ER", "cholesky"):
        acc = dict(get_loc_ms=0.0, joint_diag_ms=0.0, twin_ms=0.0, sweeps=0, twin_sweeps=0)
        after, last = [], {}
        for B in baths:
            Bl, row = device_and_twin(lib, mol, S, B, method, df=df, tensor=tensor, with_twin=method != "ER", cache=cache)      # K = naux on every bath: the twin takes minutes
            after.append(Bl)
            for k in acc:
                acc[k] += row.get(k, 0)
            if row.get("m", 0) >= last.get("m", 0):
                last = row
        out = dict(system=name, nao=mol.nao, target="bath", method=method, fragments=len(baths), bath_columns=int(sum(B.shape[1] for B in baths)),
                   possible_pairs=int(sum(B.size for B in baths)), eps=EPS, kept_pairs_before=kept(baths), kept_pairs_after=kept(after), get_loc_ms=acc["get_loc_ms"])
        if method != "cholesky":
            out.update(K=last["K"], m_max=last["m"], in_lds=last["in_lds"], converged_largest=last["converged"], sweeps=acc["sweeps"], joint_diag_ms=acc["joint_diag_ms"])
            if method != "ER":      # (no twin was run for ER on the baths: no twin fields)
                out.update(twin_ms=acc["twin_ms"], twin_sweeps=acc["twin_sweeps"])
        rows.append(out)
        print(json.dumps(rows[-1]), flush=True)
    df.free()
    mf.free()
    return rows


if __name__ == "__main__":
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "loc_bench.jsonl"
    lib = _lib.init(0)
    rows = []
    for name, mol in (("octane", Mole(ROOT / "tests" / "golden" / "octane.xyz")), ("hexadecane", Mole(alkane(16)))):
        rows += one_system(lib, name, mol)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("".join(json.dumps(r) + "\n" for r in rows))
