"""Writes tests/golden/sci_full_space_10_5.npz: the twin's run of the selection rule at (n, o) = (10, 5), eps = 1e-12, on the fragment of tests/sci_cases.py.

    python tests/golden/make_sci_full_space.py        (about a minute, 2 GB)

63 504 determinants with 876 excitations each are beyond the Python-integer loops of tests/sci_numpy.py within a test, so the run is recorded once.  The rules are
the twin's, evaluated on arrays (sci_numpy.hij_many, which tests/test_sci_hostlogic.py pins to hij); excitations come from per-string tables, membership from a
boolean array over the full space, the lowest eigenpair of each round from scipy's Lanczos on the sparse matrix of the selected space.  Recorded: the orbitals C
the run used (the set does not depend on the signs of the orbitals: |H_ai c_i| is invariant), the determinant count after every round, the margin, the final
energy, the determinants of the full space left OUTSIDE the final space, and the state before the second screen -- its space, vector and the determinants that
join -- with the eigenpair of the space that results, for checks of the single operations at this width."""
import sys
from math import comb
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sl

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent)); sys.path.insert(0, str(HERE.parent.parent)); sys.path.insert(0, str(HERE.parent.parent / "oracle"))
import fci_numpy as fnp      # noqa: E402
import sci_cases as sc       # noqa: E402
import sci_numpy as snp      # noqa: E402
from qemb_oracle import scf  # noqa: E402

N_ORB, N_OCC, EPS = 10, 5, 1e-12


def main():
    n, o = N_ORB, N_OCC
    h, e1 = sc.inputs(n, o)[:2]
    C = scf.rhf(h, e1, o, conv_tol=1e-13, conv_tol_grad=1e-10)["mo_coeff"]
    hm, Vm = C.T @ h @ C, fnp.mo_eri(e1, C)
    st = [int(s) for s in fnp.strings(n, o)]
    ns = len(st)
    pos = {s: k for k, s in enumerate(st)}
    stw = np.array(st, dtype=np.uint64)
    S = np.array([[pos[int(t)] for t in snp._targets(s, n)[0]] for s in st])      # (ns, o v): the strings one excitation away
    D = np.array([[pos[int(t)] for t in snp._targets(s, n)[1]] for s in st])      # (ns, C(o,2) C(v,2))
    full = ns * ns

    def elements(idx):
        """(source, target, H_target,source) over every excitation of the determinants idx (indices Ia * ns + Ib of the full space)"""
        src, tgt, val = [], [], []
        for k0 in range(0, len(idx), 3000):
            d = idx[k0:k0 + 3000]
            ia, ib = d // ns, d % ns
            t = np.concatenate([S[ia] * ns + ib[:, None], ia[:, None] * ns + S[ib], D[ia] * ns + ib[:, None], ia[:, None] * ns + D[ib],
                                (S[ia][:, :, None] * ns + S[ib][:, None, :]).reshape(len(d), -1)], axis=1)
            s_ = np.repeat(d, t.shape[1])
            t = t.reshape(-1)
            val.append(snp.hij_many(hm, Vm, stw[t // ns], stw[t % ns], stw[s_ // ns], stw[s_ % ns]))
            src.append(s_.astype(np.int32)); tgt.append(t.astype(np.int32))
        return np.concatenate(src), np.concatenate(tgt), np.concatenate(val)

    def lowest(idx, src, tgt, val, guess):
        where = np.full(full, -1, dtype=np.int64)
        where[idx] = np.arange(len(idx))
        keep = where[tgt] >= 0
        diag = snp.hij_many(hm, Vm, stw[idx // ns], stw[idx % ns], stw[idx // ns], stw[idx % ns])
        H = sp.coo_matrix((val[keep], (where[tgt[keep]], where[src[keep]])), shape=(len(idx),) * 2).tocsr() + sp.diags(diag)
        if len(idx) < 200:
            w, U = np.linalg.eigh(H.toarray())
        else:
            w, U = sl.eigsh(H, k=1, which="SA", v0=guess, tol=1e-14, maxiter=20000)
        c = snp.fix_sign(U[:, 0])
        assert np.linalg.norm(H @ c - w[0] * c) < 1e-10
        return float(w[0]), c

    hf = pos[(1 << o) - 1] * (ns + 1)
    idx, c = np.array([hf]), np.ones(1)
    src, tgt, val = elements(idx)
    inside = np.zeros(full, dtype=bool); inside[idx] = True
    counts, margin, e, rounds, keep = [1], np.inf, None, 0, {}
    for _ in range(30):
        cfull = np.zeros(full); cfull[idx] = c
        crit = np.abs(val * cfull[src])
        out = ~inside[tgt]
        if (out & (crit > 0)).any():
            margin = min(margin, float(np.abs(crit[out & (crit > 0)] / EPS - 1.0).min()))
        new = np.unique(tgt[out & (crit >= EPS)]).astype(np.int64)
        new = np.setdiff1d(np.union1d(new, (new % ns) * ns + new // ns), idx)
        print(f"round {rounds}: {len(idx)} determinants, {len(new)} join, margin {margin:.3e}", flush=True)
        if rounds == 1:
            keep.update(r1_idx=idx.copy(), r1_c=c.copy(), r2_joined=new.copy())
        if len(new) == 0:
            break
        rounds += 1
        s2, t2, v2 = elements(new)
        src, tgt, val = np.concatenate([src, s2]), np.concatenate([tgt, t2]), np.concatenate([val, v2])
        guess = np.zeros(full); guess[idx] = c
        idx = np.union1d(idx, new)
        inside[idx] = True
        e, c = lowest(idx, src, tgt, val, guess[idx])
        counts.append(len(idx))
        if rounds == 2:
            keep.update(r2_c=c.copy(), r2_e=e)
    outside = np.setdiff1d(np.arange(full), idx)
    key = lambda ix: np.stack([stw[ix // ns], stw[ix % ns]], axis=1)
    assert full == comb(n, o) ** 2
    np.savez_compressed(HERE / "sci_full_space_10_5.npz", n=n, o=o, eps=EPS, seed=sc.seed_of(n, o, "default"), C=C, counts=np.array(counts), rounds=rounds, margin=margin,
                        e=e, outside=key(outside), r1_keys=key(keep["r1_idx"]), r1_c=keep["r1_c"], r2_joined=key(keep["r2_joined"]), r2_c=keep["r2_c"], r2_e=keep["r2_e"])
    print(f"{len(idx)} of {full} determinants after {rounds} rounds, e = {e:.12f}, margin = {margin:.3e}, {len(outside)} outside")


if __name__ == "__main__":
    main()
