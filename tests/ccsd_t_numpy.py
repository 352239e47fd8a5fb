"""NumPy twins of the perturbative triples correction E_(T) of closed-shell CCSD with a diagonal Fock matrix (DeviceFragment.ccsd_t, fragsolver.ccsd_t), and
the two pins the twins are held to.  Integrals in chemists' notation as MO blocks: ovvv[i,a,f,b] = (ia|fb), ovoo[i,a,m,j] = (ia|mj), ovov[i,a,j,b] = (ia|jb).

    g[i,j,k,a,b,c] = sum_f (ia|fb) t2[k,j,c,f] - sum_m (ia|mj) t2[m,k,b,c]
    W = sum over the six simultaneous permutations of the pairs (i,a), (j,b), (k,c) of g
    V = W + t1[i,a] (jb|kc) + t1[j,b] (ia|kc) + t1[k,c] (ia|jb)
    r3(X)_ijk = 4 X_ijk + X_jki + X_kij - 2 X_kji - 2 X_ikj - 2 X_jik
    E_(T) = 1/3 sum W r3(V) / D,   D = e_i + e_j + e_k - e_a - e_b - e_c      (not guarded)

`full`: the o^3 v^3 tensors at once.  `tiled`: one (a, b, c) with a >= b >= c at a time with the weights 6 / 3 of the distinct arrangements (a = b = c vanishes identically), for sizes
where the full tensors are too many.  `slabbed`: one a with every (b, c) at a time, o^3 v^2 doubles live -- the twin that reaches production shapes
((21, 19) in seconds, (20, 64) in minutes).  `brute_force`: the definition, sum_T <T|H (T1 + T2)|0> <T|H T2|0> / (E0_0 - E0_T) over the triply excited determinants,
with Jordan-Wigner operators and H = sum h_pq E_pq + 1/2 sum (pq|rs) (E_pq E_rs - delta_qr E_ps); it knows nothing of the expressions above.
`two_copies`: the blocks of two non-interacting copies of a system (size consistency: twice the energy)."""
from itertools import permutations

import numpy as np


def random_system(n, o, seed, scale=0.3):
    """(h, eri, t1, t2, eo, ev): 8-fold symmetric (pq|rs), t2[i,j,a,b] = t2[j,i,b,a], orbital energies with a gap, and the h that makes the Fock matrix
    diag(eo, ev) for these integrals"""
    rng = np.random.default_rng(seed)
    v = n - o
    x = rng.standard_normal((n, n, n, n)) * scale
    x = x + x.transpose(1, 0, 2, 3)
    x = x + x.transpose(0, 1, 3, 2)
    eri = x + x.transpose(2, 3, 0, 1)
    t1 = rng.standard_normal((o, v)) * scale
    t2 = rng.standard_normal((o, o, v, v)) * scale
    t2 = t2 + t2.transpose(1, 0, 3, 2)
    eo = -1.0 - np.sort(rng.random(o))[::-1]
    ev = 1.0 + np.sort(rng.random(v))
    eps = np.concatenate([eo, ev])
    h = np.diag(eps) - 2.0 * np.einsum("pqjj->pq", eri[:, :, :o, :o]) + np.einsum("pjjq->pq", eri[:, :o, :o, :])
    return h, eri, t1, t2, eo, ev


def blocks(eri, o):
    """(ovvv, ovoo, ovov) of an n^4 tensor (pq|rs) in the MO basis"""
    return (np.ascontiguousarray(eri[:o, o:, o:, o:]), np.ascontiguousarray(eri[:o, o:, :o, :o]), np.ascontiguousarray(eri[:o, o:, :o, o:]))


def _r3(x):
    """r3 as differences, 2 (X_ijk - X_kji) + 2 (X_ijk - X_ikj) + (X_jki - X_jik) + (X_kij - X_jik): the same six coefficients, and exactly 0 at i = j = k"""
    t = lambda *p: x.transpose(*p, *range(3, x.ndim))
    return 2.0 * ((x - t(2, 1, 0)) + (x - t(0, 2, 1))) + ((t(1, 2, 0) - t(1, 0, 2)) + (t(2, 0, 1) - t(1, 0, 2)))


def full(t1, t2, ovvv, ovoo, ovov, eo, ev, skip_diagonal=True):
    """dict(e_t, abs_sum): E_(T) and 1/3 sum |W r3(V) / D|, the scale of the kernel-level bars.  skip_diagonal: the elements a = b = c, where W and V are
    invariant under every permutation of ijk and r3 of them vanishes identically, are left out (as the device does) instead of adding their rounding"""
    o, v = t1.shape
    if o == 0 or v == 0:
        return dict(e_t=0.0, abs_sum=0.0)
    g = np.einsum("iafb,kjcf->ijkabc", ovvv, t2) - np.einsum("iamj,mkbc->ijkabc", ovoo, t2)
    W = sum(g.transpose(*p, *(3 + q for q in p)) for p in permutations(range(3)))
    V = W + np.einsum("ia,jbkc->ijkabc", t1, ovov) + np.einsum("jb,iakc->ijkabc", t1, ovov) + np.einsum("kc,iajb->ijkabc", t1, ovov)
    D = (eo[:, None, None, None, None, None] + eo[None, :, None, None, None, None] + eo[None, None, :, None, None, None]
         - ev[None, None, None, :, None, None] - ev[None, None, None, None, :, None] - ev[None, None, None, None, None, :])
    terms = W * _r3(V) / D
    if skip_diagonal:
        d = np.arange(v)
        terms[:, :, :, d, d, d] = 0.0
    return dict(e_t=float(terms.sum() / 3.0), abs_sum=float(np.abs(terms).sum() / 3.0))


def tiled(t1, t2, ovvv, ovoo, ovov, eo, ev):
    """the same numbers from one (a, b, c), a >= b >= c and not a = b = c, at a time: o^3 doubles of W and V live at once"""
    o, v = t1.shape
    if o == 0 or v == 0:
        return dict(e_t=0.0, abs_sum=0.0)
    eijk = eo[:, None, None] + eo[None, :, None] + eo[None, None, :]

    def g(a, b, c):      # g[i,j,k] at the virtual indices (a, b, c)
        return np.einsum("if,kjf->ijk", ovvv[:, a, :, b], t2[:, :, c, :]) - np.einsum("imj,mk->ijk", ovoo[:, a, :, :], t2[:, :, b, c])

    e = s = 0.0
    for a in range(v):
        for b in range(a + 1):
            for c in range(b + 1):
                if a == c:
                    continue
                W = (g(a, b, c) + g(a, c, b).transpose(0, 2, 1) + g(b, a, c).transpose(1, 0, 2) + g(b, c, a).transpose(2, 0, 1)
                     + g(c, a, b).transpose(1, 2, 0) + g(c, b, a).transpose(2, 1, 0))
                V = (W + t1[:, a][:, None, None] * ovov[:, b, :, c][None, :, :] + t1[:, b][None, :, None] * ovov[:, a, :, c][:, None, :]
                     + t1[:, c][None, None, :] * ovov[:, a, :, b][:, :, None])
                terms = W * _r3(V) / (eijk - ev[a] - ev[b] - ev[c])
                w = 6.0 if a > b > c else 3.0
                e += w * terms.sum()
                s += w * np.abs(terms).sum()
    return dict(e_t=float(e / 3.0), abs_sum=float(s / 3.0))


def slabbed(t1, t2, ovvv, ovoo, ovov, eo, ev):
    """the same numbers from one virtual index a at a time, every (b, c) of it at once (the element b = c = a zeroed, as `full` does): o^3 v^2 doubles per
    tensor live, v rounds of BLAS-sized einsums -- for the shapes where `full` needs gigabytes and `tiled` millions of calls.  For fixed a the three places
    a can take in g are G1 = g[ijk,a b c], G2 = g[ijk,b a c], G3 = g[ijk,b c a], each [i,j,k,b,c], and the six arrangements of the pairs are
    W[ijk,bc] = G1[ijk,bc] + G1[ikj,cb] + G2[jik,bc] + G3[jki,bc] + G2[kij,cb] + G3[kji,cb]"""
    o, v = t1.shape
    if o == 0 or v == 0:
        return dict(e_t=0.0, abs_sum=0.0)
    ein = lambda *x: np.einsum(*x, optimize=True)
    eijk = (eo[:, None, None] + eo[None, :, None] + eo[None, None, :])[:, :, :, None, None]
    e = s = 0.0
    for a in range(v):
        G1 = ein("ifb,kjcf->ijkbc", ovvv[:, a, :, :], t2) - ein("imj,mkbc->ijkbc", ovoo[:, a, :, :], t2)
        G2 = ein("ibf,kjcf->ijkbc", ovvv[:, :, :, a], t2) - ein("ibmj,mkc->ijkbc", ovoo, t2[:, :, a, :])
        G3 = ein("ibfc,kjf->ijkbc", ovvv, t2[:, :, a, :]) - ein("ibmj,mkc->ijkbc", ovoo, t2[:, :, :, a])
        W = (G1 + G1.transpose(0, 2, 1, 4, 3) + np.einsum("jikbc->ijkbc", G2) + np.einsum("jkibc->ijkbc", G3)
             + np.einsum("kijcb->ijkbc", G2) + np.einsum("kjicb->ijkbc", G3))
        del G1, G2, G3
        V = (W + np.einsum("i,jbkc->ijkbc", t1[:, a], ovov) + np.einsum("jb,ikc->ijkbc", t1, ovov[:, a, :, :])
             + np.einsum("kc,ijb->ijkbc", t1, ovov[:, a, :, :]))
        terms = W * _r3(V) / (eijk - ev[a] - ev[:, None] - ev[None, :])
        terms[:, :, :, a, a] = 0.0
        e += terms.sum()
        s += np.abs(terms).sum()
    return dict(e_t=float(e / 3.0), abs_sum=float(s / 3.0))


def two_copies(t1, t2, ovvv, ovoo, ovov, eo, ev):
    """the amplitudes, blocks and orbital energies of two non-interacting copies: occupied orbitals [copy 1, copy 2], virtual orbitals likewise; every
    element with indices in both copies is zero"""
    o, v = t1.shape
    so, sv = (slice(0, o), slice(o, 2 * o)), (slice(0, v), slice(v, 2 * v))

    def dup(x, kinds):
        out = np.zeros(tuple(2 * d for d in x.shape))
        for c in range(2):
            out[tuple((so if k == "o" else sv)[c] for k in kinds)] = x
        return out

    return dup(t1, "ov"), dup(t2, "oovv"), dup(ovvv, "ovvv"), dup(ovoo, "ovoo"), dup(ovov, "ovov"), np.concatenate([eo, eo]), np.concatenate([ev, ev])


# ---------------------------------------------------------------- the definition, in the determinant basis
def _jw_annihilators(m):
    """a_0 .. a_{m-1} on the 2^m dimensional Fock space (Jordan-Wigner: Z on the modes before p)"""
    a1, z, i2 = np.array([[0.0, 1.0], [0.0, 0.0]]), np.diag([1.0, -1.0]), np.eye(2)
    ops = []
    for p in range(m):
        x = np.ones((1, 1))
        for q in range(m):
            x = np.kron(x, z if q < p else (a1 if q == p else i2))
        ops.append(x)
    return ops


def brute_force(h, eri, o, t1, t2, eo, ev):
    """E = sum_T <T|H (T1 + T2)|0> <T|H T2|0> / (E0_0 - E0_T) over the determinants T with three electrons moved out of |0>, T1 = sum t1[i,a] E_ai,
    T2 = 1/2 sum t2[i,j,a,b] E_ai E_bj, E0 the sum of the occupied orbital energies.  Mode 2 p + s: spatial orbital p, spin s.  n <= 5."""
    n = h.shape[0]
    v = n - o
    m = 2 * n
    a = _jw_annihilators(m)
    occ = np.array([[(d >> (m - 1 - q)) & 1 for q in range(m)] for d in range(1 << m)])      # (kron order: mode 0 is the most significant bit)
    ref = np.array([1] * (2 * o) + [0] * (2 * v))
    sector = np.where((occ[:, 0::2].sum(1) == o) & (occ[:, 1::2].sum(1) == o))[0]
    E = [[sum(a[2 * p + s].T @ a[2 * q + s] for s in range(2))[np.ix_(sector, sector)] for q in range(n)] for p in range(n)]
    dim = len(sector)
    H = np.zeros((dim, dim))
    for p in range(n):
        for q in range(n):
            H += h[p, q] * E[p][q]
            for r in range(n):
                H -= 0.5 * eri[p, q, q, r] * E[p][r]      # delta_qr E_ps: sum_q (pq|qs)
                for s in range(n):
                    H += 0.5 * eri[p, q, r, s] * (E[p][q] @ E[r][s])
    hf = np.zeros(dim)
    hf[[k for k, d in enumerate(sector) if np.array_equal(occ[d], ref)][0]] = 1.0
    T1 = sum(t1[i, x] * E[o + x][i] for i in range(o) for x in range(v))
    T2 = 0.5 * sum(t2[i, j, x, y] * (E[o + x][i] @ E[o + y][j]) for i in range(o) for j in range(o) for x in range(v) for y in range(v))
    left, right = H @ ((T1 + T2) @ hf), H @ (T2 @ hf)
    eps = np.repeat(np.concatenate([eo, ev]), 2)
    e0 = float(eps @ ref)
    e = 0.0
    for k, d in enumerate(sector):
        if int((occ[d][: 2 * o] == 0).sum()) == 3:
            e += left[k] * right[k] / (e0 - float(eps @ occ[d]))
    return float(e)
