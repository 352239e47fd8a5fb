"""NumPy restatement of what solver == "MP2" of the reference evaluates per fragment (molbe/solver.py:313-317, :781-826): PySCF's mp2.kernel,
mp2.make_rdm1, mp2.make_rdm2 (pyscf/mp/mp2.py, closed shell, no frozen orbitals, unrelaxed) and get_frag_energy (molbe/helper.py:220-339) for both
values of use_cumulant.  Dense n^4 arrays: small n only.  Test infrastructure.

PySCF is not a dependency of this repository, so the restatement is pinned by identities that fix every factor (tests/test_mp2_hostlogic.py):
Tr rdm1 = 2 o;  <h, dm1> + <eri, dm2> / 2 = E_HF + E_MP2;  dm2 - nc = the dovov part (nc: the mean-field part molbe/solver.py:513-527 subtracts for
FCI / SCI);  <eri, dovov part> / 2 = 2 E_MP2."""
import numpy as np


def mo_eri(eri1, C):
    """(pq|rs) in the MO basis from the embedding-basis tensor eri1[p,q,r,s] (chemists' notation)"""
    return np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri1, C, C, C, C, optimize=True)


def kernel(ovov, mo_energy, o):
    """mp2.kernel: t2[i,j,a,b] = (ia|jb) / (e_i + e_j - e_a - e_b), E = sum t2[ijab] (2 (ia|jb) - (ib|ja)).  ovov: [i,a,j,b]."""
    eo, ev = mo_energy[:o], mo_energy[o:]
    D = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    g = ovov.transpose(0, 2, 1, 3)                          # [i,j,a,b]
    t2 = g / D
    e = float(np.einsum("ijab,ijab->", t2, 2.0 * g - g.transpose(0, 1, 3, 2)))
    return e, t2


def theta(t2):
    """G[i,a,j,b] = 2 t2[i,j,a,b] - t2[j,i,a,b]: the layout of ovov"""
    return (2.0 * t2 - t2.transpose(1, 0, 2, 3)).transpose(0, 2, 1, 3)


def make_rdm1(t2):
    """mp2.make_rdm1 (_gamma1_intermediates): doo = -sum t2[ikab] th[jkab], dvv = sum t2[ijac] th[ijbc], th = 2 t2 - t2^T(ab);
    dm1 = [[2 I + doo + doo^T, 0], [0, dvv + dvv^T]]"""
    o, v = t2.shape[0], t2.shape[2]
    th = 2.0 * t2 - t2.transpose(0, 1, 3, 2)
    doo = -np.einsum("ikab,jkab->ij", t2, th)
    dvv = np.einsum("ijac,ijbc->ab", t2, th)
    dm1 = np.zeros((o + v, o + v))
    dm1[:o, :o] = doo + doo.T + 2.0 * np.eye(o)
    dm1[o:, o:] = dvv + dvv.T
    return dm1


def dovov_part(t2):
    """the part of mp2.make_rdm2 that is not built from 1-RDMs: dm2[i,a,j,b] = 2 (2 t2[ijab] - t2[ijba]) and its (v,o,v,o) image"""
    o, v = t2.shape[0], t2.shape[2]
    n = o + v
    d = 2.0 * (2.0 * t2.transpose(0, 2, 1, 3) - t2.transpose(0, 3, 1, 2))
    dm2 = np.zeros((n, n, n, n))
    dm2[:o, o:, :o, o:] = d
    dm2[o:, :o, o:, :o] = d.transpose(1, 0, 3, 2)
    return dm2


def mean_field_part(dm1, o):
    """`nc` of molbe/solver.py:513-527: hf (x) hf + hf (x) del + del (x) hf minus half their exchange images, hf = 2 I_occ, del = dm1 - hf"""
    hf = np.zeros_like(dm1)
    hf[np.diag_indices(o)] = 2.0
    dl = dm1 - hf
    nc = np.einsum("ij,kl->ijkl", hf, hf) + np.einsum("ij,kl->ijkl", hf, dl) + np.einsum("ij,kl->ijkl", dl, hf)
    nc -= 0.5 * (np.einsum("ij,kl->iklj", hf, hf) + np.einsum("ij,kl->iklj", hf, dl) + np.einsum("ij,kl->iklj", dl, hf))
    return nc


def make_rdm2(t2):
    """mp2.make_rdm2: the dovov part plus the terms PySCF adds from dm1 (dm2[i,i,:,:] += 2 dm1c^T, dm2[:,:,i,i] += 2 dm1c^T, dm2[:,i,i,:] -= dm1c^T,
    dm2[i,:,:,i] -= dm1c, dm1c = dm1 - 2 I_occ; dm2[i,i,j,j] += 4, dm2[i,j,j,i] -= 2)"""
    o = t2.shape[0]
    dm2 = dovov_part(t2)
    dm1c = make_rdm1(t2)
    dm1c[np.diag_indices(o)] -= 2.0
    for i in range(o):
        dm2[i, i, :, :] += 2.0 * dm1c.T
        dm2[:, :, i, i] += 2.0 * dm1c.T
        dm2[:, i, i, :] -= dm1c.T
        dm2[i, :, :, i] -= dm1c
    for i in range(o):
        for j in range(o):
            dm2[i, i, j, j] += 4.0
            dm2[i, j, j, i] -= 2.0
    return dm2


def get_frag_energy(C, o, n_frag, weight, centers, h1, rdm1_mo, rdm2_mo, eri1, veff0=None, veff=None, use_cumulant=True):
    """molbe/helper.py:278-339 with the fragment ERIs as the dense tensor eri1[p,q,r,s]: [e1, e2, ec] (weighted centre sums)"""
    rdm1 = C @ rdm1_mo @ C.T * 0.5
    hf = C[:, :o] @ C[:, :o].T
    if use_cumulant:
        d = 2.0 * (rdm1 - hf)
        e1 = np.einsum("ij,ij->i", h1[:n_frag], d[:n_frag])
        ec = np.einsum("ij,ij->i", veff0[:n_frag], d[:n_frag])
    else:
        e1 = 2.0 * np.einsum("ij,ij->i", h1[:n_frag], rdm1[:n_frag])
        ec = np.einsum("ij,ij->i", veff[:n_frag], rdm1[:n_frag])
    r2 = np.einsum("ijkl,pi,qj,rk,sl->pqrs", 0.5 * rdm2_mo, C, C, C, C, optimize=True)
    # helper.py:315-321: e2_i = sum_j sum_{k,l} G[i,j,k,l] (ij|kl), the packed (k >= l) sum written out
    e2 = np.einsum("ijkl,ijkl->i", r2[:n_frag], eri1[:n_frag])
    return np.array([weight * sum(e1[c] for c in centers), weight * sum(e2[c] for c in centers), weight * sum(ec[c] for c in centers)])


def fragment_mp2(C, mo_energy, o, eri1, n_frag=0, weight=1.0, centers=(), h1=None, veff0=None, veff=None, use_cumulant=True):
    """everything the device returns for one fragment, from the orbitals it returned: dict(e_corr, t2, rdm1_mo, rdm1_emb, e_frag).
    use_cumulant=True contracts the cumulant of the MP2 2-RDM (its dovov part); False the full make_rdm2, the reference's literal expression."""
    n = C.shape[0]
    if o == n:
        t2 = np.zeros((o, o, 0, 0)); e = 0.0
    else:
        ovov = mo_eri(eri1, C)[:o, o:, :o, o:]
        e, t2 = kernel(ovov, mo_energy, o)
    dm1 = make_rdm1(t2)
    out = dict(e_corr=e, t2=t2, rdm1_mo=dm1, rdm1_emb=C @ dm1 @ C.T * 0.5)
    if h1 is not None:
        dm2 = dovov_part(t2) if use_cumulant else make_rdm2(t2)
        out["e_frag"] = get_frag_energy(C, o, n_frag, weight, centers, h1, dm1, dm2, eri1, veff0, veff, use_cumulant)
    return out
