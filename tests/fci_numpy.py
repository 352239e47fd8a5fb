"""NumPy reference of the determinant-space FCI behind solver="FCI-hip" (test infrastructure).

Two independent forms of the same Hamiltonian H = sum h_pq a+_p a_q + 1/2 sum (pq|rs) a+_p a+_r a_s a_q over M_s = 0 determinants |Ia Ib> (alpha string slow,
strings in ascending order of their bit patterns, the alpha creators to the left of the beta ones):
* brute force: every term applied to every determinant as creation / annihilation operators on spin-orbital bit strings with explicit fermion signs -> the dense
  matrix -> numpy.linalg.eigh.  No E_pq, no link table, no Knowles-Handy rearrangement.
* string-space operators: the matrices A_pq of E_pq on ONE spin's strings, E^alpha c = A c and E^beta c = c A^T on the (ns, ns) vector.  Gives sigma and the RDMs at
  sizes where the dense matrix does not fit.
Conventions are PySCF's: dm1[p,q] = <q+ p> (symmetric here), dm2[p,q,r,s] = <p+ r+ s q>, E = sum h dm1 + 1/2 sum (pq|rs) dm2."""
from functools import lru_cache
from math import comb

import numpy as np


def strings(n, k):
    return np.array([s for s in range(1 << n) if bin(s).count("1") == k], dtype=np.int64)


# ---------------------------------------------------------------- brute force: operators on spin-orbital bit strings
def hamiltonian_matrix(h, V, k):
    """dense H over the C(n,k)^2 determinants; spin orbital i < n: alpha orbital i, n + i: beta orbital i"""
    n = h.shape[0]
    st = strings(n, k)
    ns = len(st)
    pos = np.full(1 << n, -1, dtype=np.int64)
    pos[st] = np.arange(ns)
    masks0 = (st[:, None] | (st[None, :] << n)).reshape(-1)            # index Ia * ns + Ib
    parity = np.array([bin(m).count("1") & 1 for m in range(1 << (2 * n))], dtype=np.int64)
    N = ns * ns
    H = np.zeros((N, N))
    col = np.arange(N)

    def annihilate(m, sg, ok, i):
        ok = ok & (((m >> i) & 1) == 1)
        sg = sg * (1 - 2 * parity[m & ((1 << i) - 1)])
        return m & ~(1 << i), sg, ok

    def create(m, sg, ok, i):
        ok = ok & (((m >> i) & 1) == 0)
        sg = sg * (1 - 2 * parity[m & ((1 << i) - 1)])
        return m | (1 << i), sg, ok

    def add(m, sg, ok, coef):
        row = pos[m[ok] & ((1 << n) - 1)] * ns + pos[m[ok] >> n]
        np.add.at(H, (row, col[ok]), coef * sg[ok])

    one = np.ones(N, dtype=np.int64)
    yes = np.ones(N, dtype=bool)
    for s1 in (0, n):
        for p in range(n):
            for q in range(n):
                m, sg, ok = annihilate(masks0, one, yes, s1 + q)
                m, sg, ok = create(m, sg, ok, s1 + p)
                add(m, sg, ok, h[p, q])
                for s2 in (0, n):
                    for r in range(n):
                        for s in range(n):      # a+_p a+_r a_s a_q, rightmost first
                            m, sg, ok = annihilate(masks0, one, yes, s1 + q)
                            m, sg, ok = annihilate(m, sg, ok, s2 + s)
                            m, sg, ok = create(m, sg, ok, s2 + r)
                            m, sg, ok = create(m, sg, ok, s1 + p)
                            add(m, sg, ok, 0.5 * V[p, q, r, s])
    return H


def fix_sign(c):
    """normalised, the largest-magnitude component positive (ties: the lowest index)"""
    c = np.asarray(c, dtype=float)
    c = c / np.linalg.norm(c)
    i = int(np.argmax(np.abs(c.reshape(-1))))
    return c if c.reshape(-1)[i] > 0 else -c


def ground_state(h, V, k):
    """(E, c (ns, ns)) by eigh of the brute-force matrix"""
    H = hamiltonian_matrix(h, V, k)
    w, U = np.linalg.eigh(H)
    ns = comb(h.shape[0], k)
    return w[0], fix_sign(U[:, 0]).reshape(ns, ns), H


# ---------------------------------------------------------------- string-space operators
@lru_cache(maxsize=None)
def e_matrices(n, k):
    """A[p*n+q] (ns, ns): <I|E_pq|J> on one spin's strings, built by applying a_q then a+_p to every string"""
    st = strings(n, k)
    ns = len(st)
    pos = {int(s): i for i, s in enumerate(st)}
    A = np.zeros((n * n, ns, ns))
    for J, s in enumerate(st):
        s = int(s)
        for q in range(n):
            if not (s >> q) & 1:
                continue
            sg = -1 if bin(s & ((1 << q) - 1)).count("1") & 1 else 1
            t = s & ~(1 << q)
            for p in range(n):
                if (t >> p) & 1:
                    continue
                sg2 = -sg if bin(t & ((1 << p) - 1)).count("1") & 1 else sg
                A[p * n + q, pos[t | (1 << p)], J] = sg2
    return A


def d_tensor(c, n, k):
    """D[pq] = E_pq c = A_pq c + c A_pq^T, (n^2, ns, ns)"""
    A = e_matrices(n, k)
    return A @ c + c @ A.transpose(0, 2, 1)


def sigma(h, V, c, k):
    """H c in the operator form: H = sum k_pq E_pq + 1/2 sum (pq|rs) E_pq E_rs, k_pq = h_pq - 1/2 sum_r (pr|rq)"""
    n = h.shape[0]
    A = e_matrices(n, k)
    kk = (h - 0.5 * np.einsum("prrq->pq", V)).reshape(-1)
    D = d_tensor(c, n, k)
    G = np.tensordot(V.reshape(n * n, n * n), D, axes=([1], [0]))
    s = np.tensordot(kk, D, axes=([0], [0]))
    s += 0.5 * ((A @ G).sum(axis=0) + (G @ A.transpose(0, 2, 1)).sum(axis=0))
    return s


def rdm12(c, n, k):
    """(dm1, dm2) of the vector c, PySCF conventions"""
    D = d_tensor(c, n, k).reshape(n * n, -1)
    dm1 = (D @ c.reshape(-1)).reshape(n, n)
    dm1 = 0.5 * (dm1 + dm1.T)
    A = (D @ D.T).reshape(n, n, n, n)                      # A[p,q,r,s] = <E_qp E_rs>
    dm2 = A.transpose(1, 0, 2, 3).copy()
    for q in range(n):
        dm2[:, q, q, :] -= dm1
    return dm1, dm2


def mean_field_part(dm1, k):
    """nc of molbe/solver.py:513-527"""
    hf = np.zeros_like(dm1)
    hf[np.diag_indices(k)] = 2.0
    d = dm1 - hf
    nc = np.einsum("ij,kl->ijkl", hf, hf) + np.einsum("ij,kl->ijkl", hf, d) + np.einsum("ij,kl->ijkl", d, hf)
    nc -= 0.5 * (np.einsum("ij,kl->iklj", hf, hf) + np.einsum("ij,kl->iklj", hf, d) + np.einsum("ij,kl->iklj", d, hf))
    return nc


def mo_eri(e1, C):
    return np.einsum("ijkl,ip,jq,kr,ls->pqrs", e1, C, C, C, C, optimize=True)


def energy_from_rdms(h, V, dm1, dm2):
    return float(np.einsum("pq,pq->", h, dm1) + 0.5 * np.einsum("pqrs,pqrs->", V, dm2))
