"""Integral source + mean-field for real molecules without PySCF.

`Mole` / `RHF` expose the handful of PySCF attributes `BE` reads (molbe/mbe.py:361-373): `mol.nelectron`,
`mo_coeff`, `mo_energy`, `e_tot`, `_eri`, `energy_nuc()`, `get_hcore()`, `get_ovlp()`, `make_rdm1()`,
`get_veff()`, plus the shell queries the semi-sparse DF pipeline uses (molbe/eri_sparse_DF.py: `nbas`, `ao_loc_nr`, `bas_angular`,
`bas_exp`, `bas_coord`).  Integrals come from the in-tree host library libqemb_gto.so (csrc_host/gto_ints.c, McMurchie-Davidson over
Cartesian Gaussians: s, p, d orbital shells, auxiliary shells up to g); shells with l >= 2 are used as real solid harmonics like
PySCF's default (`cart=False`): the Cartesian integrals are contracted with a per-shell Cartesian -> spherical matrix.
Built-in orbital bases: STO-3G for H and C (the reference's test systems), cc-pVDZ for H; any basis can be passed as a dict
{symbol: [(l, exponents, coefficients), ...]}.  `etb_auxbasis` generates an even-tempered auxiliary basis -- the image holds no basis-set
library, so the reference's `weigend` (def2-universal-jfit) fitting basis is not available.
This is upstream of the hot path -- CPU work in the reference too (libcint) -- and exists so that the reference's
end-to-end golden energies can be reproduced from first principles.
"""

from __future__ import annotations

import ctypes as C
import itertools
from pathlib import Path

import numpy as np

BOHR = 0.52917721092            # Angstrom per Bohr (pyscf.data.nist.BOHR)
_HERE = Path(__file__).resolve().parent
GTO_LIB = _HERE / "libqemb_gto.so"
MAXPRIM = 8
_L = {"s": 0, "p": 1, "d": 2, "f": 3, "g": 4}

# STO-3G (EMSL / PySCF 'sto-3g'): (l, exponents, coefficients) per shell; 'sp' shells share exponents
_STO3G = {
    "H": [("s", [3.42525091, 0.62391373, 0.16885540], [0.15432897, 0.53532814, 0.44463454])],
    "C": [("s", [71.6168370, 13.0450960, 3.5305122], [0.15432897, 0.53532814, 0.44463454]),
          ("s", [2.9412494, 0.6834831, 0.2222899], [-0.09996723, 0.39951283, 0.70011547]),
          ("p", [2.9412494, 0.6834831, 0.2222899], [0.15591627, 0.60768372, 0.39195739])],
}
# cc-pVDZ, hydrogen only (2s1p; EMSL / PySCF 'cc-pvdz'): a multi-AO-per-atom test basis for the s/p generator
_CCPVDZ = {
    "H": [("s", [13.0100000, 1.9620000, 0.4446000], [0.0196850, 0.1379770, 0.4781480]),
          ("s", [0.1220000], [1.0]),
          ("p", [0.7270000], [1.0])],
}
_BASES = {"sto-3g": _STO3G, "cc-pvdz": _CCPVDZ}
_Z = {"H": 1, "C": 6}


class _BF(C.Structure):
    _fields_ = [("ctr", C.c_double * 3), ("lmn", C.c_int * 3), ("nprim", C.c_int), ("ex", C.c_double * MAXPRIM),
                ("co", C.c_double * MAXPRIM)]


def _dfact(n):
    return 1.0 if n <= 0 else float(np.prod(np.arange(n, 0, -2)))


def _load():
    if not GTO_LIB.exists():
        raise RuntimeError(f"{GTO_LIB} not found: build with __graft_entry__.build()")
    lib = C.CDLL(str(GTO_LIB))
    lib.gto_bf_size.restype = C.c_size_t
    assert lib.gto_bf_size() == C.sizeof(_BF)
    return lib


def read_xyz(path):
    lines = Path(path).read_text().strip().splitlines()
    n = int(lines[0])
    atoms = []
    for ln in lines[2: 2 + n]:
        s = ln.split()
        atoms.append((s[0], tuple(float(x) for x in s[1:4])))
    return atoms


def cart_components(l):
    """Cartesian monomial exponents of a shell in PySCF / libcint order: xx xy xz yy yz zz for l = 2, ..."""
    return [(lx, ly, l - lx - ly) for lx in range(l, -1, -1) for ly in range(l - lx, -1, -1)]


def cart2sph(l):
    """(ncart, 2l+1): real solid harmonics of degree l as combinations of the shell's Cartesian functions, for Cartesian functions
    that share ONE radial normalisation (the x^l component has unit norm).  The 2l+1 harmonic polynomials are the null space of the
    Laplacian on the degree-l monomials; the columns are orthonormalised under the Gaussian overlap metric of those monomials,
    <x^a y^b z^c | x^d y^e z^f> = (a+d-1)!! (b+e-1)!! (c+f-1)!! / (2l-1)!! for all-even sums.  Any orthonormal basis of that space gives
    the same fitted integrals (the density-fitting sums are invariant under rotations inside a shell); s and p are the identity."""
    comps = cart_components(l)
    nc = len(comps)
    if l <= 1:
        return np.eye(nc)
    lower = {c: i for i, c in enumerate(cart_components(l - 2))}
    Lap = np.zeros((len(lower), nc))
    for j, c in enumerate(comps):
        for d in range(3):
            if c[d] >= 2:
                cc = list(c); cc[d] -= 2
                Lap[lower[tuple(cc)], j] += c[d] * (c[d] - 1)
    _, sv, Vt = np.linalg.svd(Lap)
    null = Vt[len(lower):].T if len(lower) < nc else Vt[(sv > 1e-12).sum():].T           # nc x (2l+1)
    assert null.shape[1] == 2 * l + 1
    G = np.zeros((nc, nc))
    for i, a in enumerate(comps):
        for j, b in enumerate(comps):
            if all((a[d] + b[d]) % 2 == 0 for d in range(3)):
                G[i, j] = np.prod([_dfact(a[d] + b[d] - 1) for d in range(3)]) / _dfact(2 * l - 1)
    # Loewdin orthonormalisation under G: columns X with X^T G X = 1
    M = null.T @ G @ null
    w, U = np.linalg.eigh(M)
    return null @ (U / np.sqrt(w)) @ U.T


class Mole:
    def __init__(self, atom, basis="sto-3g", unit="Angstrom"):
        if isinstance(basis, str):
            if basis.lower() not in _BASES:
                raise NotImplementedError("built-in bases: STO-3G (H, C), cc-pVDZ (H); pass a dict {symbol: [(l, exps, coefs), ...]} otherwise")
            table = _BASES[basis.lower()]
        else:
            table = basis
        self.basis = basis
        if isinstance(atom, (str, Path)):
            atom = read_xyz(atom)
        scale = 1.0 / BOHR if unit.lower().startswith("a") else 1.0
        self.atom = [(sym, tuple(scale * np.asarray(xyz, dtype=float))) for sym, xyz in atom]
        self.nelectron = sum(_Z[s] for s, _ in self.atom)
        self.bfs = []          # Cartesian contracted functions handed to libqemb_gto
        self.ao_atom = []      # atom of every (spherical) AO
        self.shells = []       # (atom, l, exponents, coefficients, first AO, first Cartesian function)
        blocks = []
        for ia, (sym, xyz) in enumerate(self.atom):
            if sym not in table:
                raise NotImplementedError(f"no basis for {sym} in the table given")
            for l, exps, coefs in table[sym]:
                l = _L[l] if isinstance(l, str) else int(l)
                if l > 4:
                    raise NotImplementedError("shells beyond g are not supported")
                self.shells.append((ia, l, np.asarray(exps, dtype=float), np.asarray(coefs, dtype=float), len(self.ao_atom), len(self.bfs)))
                for lmn in cart_components(l):
                    self.bfs.append(self._make_bf(xyz, lmn, exps, coefs, common=(l >= 2)))
                blocks.append(cart2sph(l))
                self.ao_atom += [ia] * (2 * l + 1)
        self.ncart = len(self.bfs)
        self.nao = len(self.ao_atom)
        self.cart = all(b.shape[0] == b.shape[1] for b in blocks)      # only s and p shells: Cartesian == spherical
        self.c2s = np.zeros((self.ncart, self.nao))
        r = c = 0
        for b in blocks:
            self.c2s[r: r + b.shape[0], c: c + b.shape[1]] = b
            r += b.shape[0]; c += b.shape[1]

    @staticmethod
    def _make_bf(xyz, lmn, exps, coefs, common=False):
        """One Cartesian contracted Gaussian.  common=False (s, p): unit self-overlap.  common=True (l >= 2): every component of the
        shell carries the normalisation of its x^l component, the convention `cart2sph` assumes."""
        L = sum(lmn)
        nl = (L, 0, 0) if common else lmn
        e = np.asarray(exps, dtype=float); c = np.asarray(coefs, dtype=float)
        norm = (2 * e / np.pi) ** 0.75 * (4 * e) ** (L / 2.0) / np.sqrt(_dfact(2 * nl[0] - 1) * _dfact(2 * nl[1] - 1) * _dfact(2 * nl[2] - 1))
        cc = c * norm
        # renormalise the contraction to unit self-overlap
        pref = np.pi ** 1.5 * _dfact(2 * nl[0] - 1) * _dfact(2 * nl[1] - 1) * _dfact(2 * nl[2] - 1) / 2.0 ** L
        s = sum(cc[i] * cc[j] * pref / (e[i] + e[j]) ** (L + 1.5) for i in range(len(e)) for j in range(len(e)))
        cc = cc / np.sqrt(s)
        if len(e) > MAXPRIM:
            raise NotImplementedError(f"at most {MAXPRIM} primitives per contraction")
        b = _BF()
        b.ctr[:] = xyz; b.lmn[:] = lmn; b.nprim = len(e)
        for i in range(len(e)):
            b.ex[i] = e[i]; b.co[i] = cc[i]
        return b

    def _arr(self):
        return (_BF * self.ncart)(*self.bfs)

    # ---- shell queries (the PySCF names the reference's eri_sparse_DF.py uses) -----------------------------------------------
    @property
    def natm(self):
        return len(self.atom)

    @property
    def nbas(self):
        return len(self.shells)

    def ao_loc_nr(self):
        return np.array([sh[4] for sh in self.shells] + [self.nao])

    def bas_angular(self, i):
        return self.shells[i][1]

    def bas_exp(self, i):
        return self.shells[i][2]

    def bas_ctr_coeff(self, i):
        return self.shells[i][3]

    def bas_atom(self, i):
        return self.shells[i][0]

    def bas_coord(self, i):
        return np.asarray(self.atom[self.shells[i][0]][1])

    def atom_charge(self, ia):
        return _Z[self.atom[ia][0]]

    def aoslice_by_atom(self):
        """PySCF's (shell0, shell1, ao0, ao1) per atom."""
        ao = np.asarray(self.ao_atom)
        sh = np.asarray([s[0] for s in self.shells])
        out = []
        for ia in range(self.natm):
            w = np.nonzero(ao == ia)[0]
            ws = np.nonzero(sh == ia)[0]
            out.append((int(ws[0]), int(ws[-1]) + 1, int(w[0]), int(w[-1]) + 1))
        return np.array(out)

    def energy_nuc(self):
        e = 0.0
        for i, (si, xi) in enumerate(self.atom):
            for sj, xj in self.atom[:i]:
                e += _Z[si] * _Z[sj] / np.linalg.norm(np.asarray(xi) - np.asarray(xj))
        return e

    # ---- integrals ---------------------------------------------------------------------------------------------------------
    def _sph2(self, X):
        return X if self.cart else self.c2s.T @ X @ self.c2s

    def one_electron(self):
        lib = _load()
        n = self.ncart
        S = np.zeros((n, n)); T = np.zeros((n, n)); V = np.zeros((n, n))
        xyz = np.ascontiguousarray([a[1] for a in self.atom], dtype=float)
        Z = np.ascontiguousarray([_Z[a[0]] for a in self.atom], dtype=float)
        lib.gto_one_electron(n, self._arr(), len(self.atom), xyz.ctypes.data_as(C.c_void_p), Z.ctypes.data_as(C.c_void_p),
                             S.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p))
        return self._sph2(S), self._sph2(T), self._sph2(V)

    def dipole(self, origin=(0.0, 0.0, 0.0)):
        """<a|r - origin|b>: (3, nao, nao), from the host library (gto_dipole)"""
        lib = _load()
        n = self.ncart
        out = np.zeros((3, n, n))
        o = np.ascontiguousarray(origin, dtype=float)
        if o.shape != (3,):
            raise ValueError("origin: three Cartesian coordinates (Bohr)")
        lib.gto_dipole(n, self._arr(), o.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        out = np.array([self._sph2(x) for x in out])
        return 0.5 * (out + out.transpose(0, 2, 1))      # the Cartesian blocks are symmetric to the bit; the product with c2s is made so again

    def eri_s1(self):
        lib = _load()
        n = self.ncart
        out = np.zeros((n, n, n, n))
        lib.gto_eri_s1(n, self._arr(), out.ctypes.data_as(C.c_void_p))
        if not self.cart:
            c = self.c2s
            out = np.einsum("pqrs,pi,qj,rk,sl->ijkl", out, c, c, c, c, optimize=True)
        return out

    def intor(self, name):
        if name == "int1e_ovlp":
            return self.one_electron()[0]
        if name == "int2c2e":
            return int2c2e(self)
        raise NotImplementedError(name)


# ---- auxiliary basis and the 2- / 3-centre Coulomb integrals of density fitting ---------------------------------------------
def etb_auxbasis(mol: Mole, beta=2.0, lmax=None, lmax_by_symbol=None):
    """An even-tempered auxiliary basis in the spirit of PySCF's `df.addons.aug_etb`: for every element and every auxiliary angular
    momentum L up to twice the largest orbital l (capped at `lmax`), uncontracted exponents emin * beta^k covering the range of the
    orbital-PRODUCT exponents a_i + a_j of the shell pairs (l_i, l_j) that can couple to L.  Returned as a basis dict for `Mole`."""
    out = {}
    for sym in sorted(set(s for s, _ in mol.atom)):
        ia = next(i for i, (s, _) in enumerate(mol.atom) if s == sym)
        shells = [(sh[1], sh[2]) for sh in mol.shells if sh[0] == ia]
        lo = max(l for l, _ in shells)
        Lmax = 2 * lo if lmax is None else min(2 * lo, lmax)
        if lmax_by_symbol and sym in lmax_by_symbol:
            Lmax = lmax_by_symbol[sym]
        basis = []
        for L in range(Lmax + 1):
            sums = [a + b for (li, ei), (lj, ej) in itertools.product(shells, shells) if abs(li - lj) <= L <= li + lj for a in ei for b in ej]
            if not sums:       # no orbital pair of this element reaches L (e.g. polarisation functions for a minimal basis): reuse L - 1
                sums = prev
            emin, emax = min(sums), max(sums)
            nexp = max(1, int(np.ceil(np.log(emax / emin) / np.log(beta))) + 1)
            basis += [(L, [emin * beta ** k], [1.0]) for k in range(nexp)]
            prev = sums
        out[sym] = basis
    return out


def make_auxmol(mol: Mole, auxbasis):
    """pyscf.df.addons.make_auxmol: the same atoms carrying the auxiliary basis (a dict, or "etb" / ("etb", beta, lmax))."""
    if isinstance(auxbasis, str):
        if auxbasis.lower() != "etb":
            raise NotImplementedError(f"auxiliary basis {auxbasis!r}: the image holds no basis-set library (no PySCF, no network); "
                                      "pass a basis dict or 'etb' (even-tempered, generated from the orbital basis)")
        auxbasis = etb_auxbasis(mol)
    elif isinstance(auxbasis, tuple) and auxbasis[0] == "etb":
        auxbasis = etb_auxbasis(mol, *auxbasis[1:])
    aux = Mole(mol.atom, basis=auxbasis, unit="Bohr")
    return aux


def _backend(backend):
    if backend not in ("host", "hip"):
        raise ValueError(f"backend {backend!r}: 'host' (libqemb_gto, the default) or 'hip' (the device kernels of libqemb_hip)")
    return backend == "hip"


def c2s_table():
    """The Cartesian -> spherical matrices of l = 0..4 one after the other (245 doubles): what qemb_int_basis_create uploads."""
    return np.ascontiguousarray(np.concatenate([cart2sph(l).ravel() for l in range(5)]))


class DeviceBasis:
    """A basis uploaded once to the device (qemb_int_basis_create) in the record format of `Mole.bfs`; freed on __del__ / .free()."""

    def __init__(self, mol: Mole, lib=None):
        from . import _lib
        self.lib = lib or _lib.init()
        h = C.c_void_p()
        arr, tab = mol._arr(), c2s_table()
        _lib.check(self.lib.qemb_int_basis_create(mol.ncart, C.addressof(arr), C.sizeof(_BF), tab.ctypes.data, C.byref(h)), "qemb_int_basis_create", self.lib)
        self.h, self.nao = h, mol.nao
        self._xyz = np.ascontiguousarray([a[1] for a in mol.atom], dtype=float).reshape(-1, 3)
        self._Z = np.ascontiguousarray([_Z[a[0]] for a in mol.atom], dtype=float)

    def one_electron(self):
        """(S, T, V) of the basis from the device kernel (qemb_int1e): overlap, kinetic energy and nuclear attraction sum_C -Z_C <a|1/r_C|b> over the atoms of the
        molecule the basis was made from -- the arrays of `Mole.one_electron()`.  Symmetric to the bit; two calls return the same bits."""
        from . import _lib
        N = self.nao
        S, T, V = np.empty((N, N)), np.empty((N, N)), np.empty((N, N))
        _lib.check(self.lib.qemb_int1e(self.h, len(self._Z), self._xyz.ctypes.data, self._Z.ctypes.data, S.ctypes.data, T.ctypes.data, V.ctypes.data), "qemb_int1e", self.lib)
        return S, T, V

    def dipole(self, origin=(0.0, 0.0, 0.0)):
        """<a|r - origin|b> from the device kernel (qemb_int1e_dipole): (3, N, N), the arrays of `Mole.dipole()`.  Symmetric to the bit."""
        from . import _lib
        o = np.ascontiguousarray(origin, dtype=float)
        if o.shape != (3,):
            raise ValueError("origin: three Cartesian coordinates (Bohr)")
        out = np.empty((3, self.nao, self.nao))
        _lib.check(self.lib.qemb_int1e_dipole(self.h, o.ctypes.data, out.ctypes.data), "qemb_int1e_dipole", self.lib)
        return out

    def eri(self, sym=8, thresh=0.0, out_dev=None):
        """(mu nu|la si) from the device kernels (qemb_int4c2e) in form `sym`: 8 (1-D, PySCF's 8-fold packed form), 4 ([npair][npair]) or 1 ([N]^4).  out_dev: a
        device pointer the integrals are left at (nothing is copied to the host; returns None); otherwise a host array."""
        from . import _lib
        if sym not in (1, 4, 8):
            raise ValueError("sym must be 1, 4 or 8")
        N = self.nao
        npair = N * (N + 1) // 2
        if out_dev is not None:
            _lib.check(self.lib.qemb_int4c2e(self.h, int(sym), float(thresh), out_dev, 1), "qemb_int4c2e", self.lib)
            return None
        out = np.empty({8: (npair * (npair + 1) // 2,), 4: (npair, npair), 1: (N,) * 4}[sym])
        _lib.check(self.lib.qemb_int4c2e(self.h, int(sym), float(thresh), out.ctypes.data, 0), "qemb_int4c2e", self.lib)
        return out

    def eri_stats(self):
        """(canonical shell quartets, of which screened) of the last four-centre fill of this basis"""
        n, z = C.c_int64(), C.c_int64()
        from . import _lib
        _lib.check(self.lib.qemb_int4c_stats(self.h, C.byref(n), C.byref(z)), "qemb_int4c_stats", self.lib)
        return n.value, z.value

    def get_jk(self, dm, thresh=0.0, with_j=True, with_k=True):
        """Integral-direct J[mu,nu] = sum (mu nu|la si) D[la,si] and K[mu,la] = sum (mu nu|la si) D[nu,si] for a symmetric `dm` (qemb_int_jk_direct): the shell
        quartets are evaluated on the device and contracted with the density where they were evaluated, no integral is stored.  The first call writes the pair
        stage and the Schwarz factors and keeps them on the device with this object; later calls reuse them.  thresh > 0 skips a quartet with Q_ab Q_cd < thresh
        or Q_ab Q_cd max|D| < thresh (`eri_stats()` counts them).  Returns (J, K); a matrix that was not asked for is None.  J and K are symmetric to the bit,
        but their sums are accumulated with FP64 atomic adds: unlike the stored integrals of `eri()` the last bits may differ from run to run."""
        from . import _lib
        if not (with_j or with_k):
            raise ValueError("get_jk: with_j and with_k are both False")
        N = self.nao
        dm = _symmetric_density(dm, N)
        J = np.empty((N, N)) if with_j else None
        K = np.empty((N, N)) if with_k else None
        _lib.check(self.lib.qemb_int_jk_direct(self.h, dm.ctypes.data, float(thresh), J.ctypes.data if with_j else None, K.ctypes.data if with_k else None, 0),
                   "qemb_int_jk_direct", self.lib)
        return J, K

    def jk_bytes(self):
        """device bytes a get_jk call of this basis takes (pair stage, lists, O(N^2)): qemb_int_jk_direct_bytes"""
        from . import _lib
        n = C.c_int64()
        _lib.check(self.lib.qemb_int_jk_direct_bytes(self.h, C.byref(n)), "qemb_int_jk_direct_bytes", self.lib)
        return n.value

    def ao2mo(self, TAs, frags=None, want_host=True, tile_pairs=None, thresh=0.0):
        """Integral-direct AO -> fragment transform (qemb_ao2mo_direct): the 4-fold packed fragment integrals of `AOEri.transform` for every coefficient matrix
        of `TAs` (each N x n_f) from ONE pass over the integrals, which are evaluated tile by tile and never stored -- device memory is
        O(tile^2 + tile n^2 + sum_f npair(n_f)^2), nothing grows as N^4.  frags: fragment handles (DeviceFragment, or None) the blocks go straight into;
        want_host: also return them as host arrays.  tile_pairs: AO pairs per tile (None: chosen from the free device memory).  thresh > 0: Schwarz screening
        of quartets and of whole tiles (`eri_stats()`, `tile_stats()`).  Returns a list of (npair(n_f), npair(n_f)) arrays, or None with want_host=False.
        Bit-reproducible from run to run and exactly symmetric."""
        from . import _lib
        TAs = [np.ascontiguousarray(t, dtype=np.float64) for t in TAs]
        nf = len(TAs)
        if nf == 0:
            raise ValueError("ao2mo: no coefficient matrix")
        if any(t.ndim != 2 or t.shape[0] != self.nao for t in TAs):
            raise ValueError(f"ao2mo: every TA must have {self.nao} rows")
        if frags is not None and len(frags) != nf:
            raise ValueError("ao2mo: one fragment handle (or None) per coefficient matrix")
        ns = (C.c_int * nf)(*[t.shape[1] for t in TAs])
        ta = (C.c_void_p * nf)(*[t.ctypes.data for t in TAs])
        outs = [np.empty((n * (n + 1) // 2,) * 2) for n in ns] if want_host else None
        op = (C.c_void_p * nf)(*[o.ctypes.data for o in outs]) if want_host else None
        fh = None if frags is None else (C.c_void_p * nf)(*[None if f is None else f.h.value for f in frags])
        _lib.check(self.lib.qemb_ao2mo_direct(self.h, nf, ta, ns, op, fh, int(tile_pairs or 0), float(thresh)), "qemb_ao2mo_direct", self.lib)
        return outs

    def ao2mo_bytes(self, ns, tile_pairs=None):
        """device bytes an `ao2mo` call for fragments of `ns` embedding orbitals takes at this tile size (qemb_ao2mo_direct_bytes): the figure the call checks
        against the free memory and the limit of qemb_int4c_mem_limit before it allocates anything"""
        from . import _lib
        ns = [int(n) for n in ns]
        arr, b = (C.c_int * len(ns))(*ns), C.c_int64()
        _lib.check(self.lib.qemb_ao2mo_direct_bytes(self.h, len(ns), arr, int(tile_pairs or 0), C.byref(b)), "qemb_ao2mo_direct_bytes", self.lib)
        return b.value

    def tile_stats(self):
        """(tiles visited, tiles skipped) of the last `ao2mo` call of this basis"""
        from . import _lib
        v, z = C.c_int64(), C.c_int64()
        _lib.check(self.lib.qemb_int4c_tile_stats(self.h, C.byref(v), C.byref(z)), "qemb_int4c_tile_stats", self.lib)
        return v.value, z.value

    def cholesky(self, tol=1e-8, span=0.01, panel_pairs=None, max_rank=None):
        """Pivoted, incomplete Cholesky decomposition of the AO integrals on the device (qemb_int_cholesky): an (M, npair) array L in canonical packed order with
        max |(ij|kl) - sum_K L[K,ij] L[K,kl]| <= tol, from M npair integrals instead of npair^2 / 2 and with no auxiliary basis.  span: a panel takes the shell
        pairs whose largest residual diagonal exceeds max(span max d, tol); panel_pairs: AO pairs per panel (None: 128); max_rank: the most vectors the factor
        may have (None: what the device memory allows, at most npair) -- a decomposition that needs more raises QembError (QEMB_ERR_NOCONV) instead of
        returning a worse factor.  The same bits on every call; `cholesky_stats()` afterwards.  (The host buffer has room for max_rank rows: for large systems
        keep the factor on the device with eri_transform.DFContext.from_cholesky.)"""
        from . import _lib
        npair = self.nao * (self.nao + 1) // 2
        rows = npair if not max_rank else min(int(max_rank), npair)
        out, m = np.empty((rows, npair)), C.c_int64()
        _lib.check(self.lib.qemb_int_cholesky(self.h, float(tol), float(span), int(panel_pairs or 0), int(max_rank or 0), out.ctypes.data, C.byref(m)),
                   "qemb_int_cholesky", self.lib)
        return np.ascontiguousarray(out[: m.value])

    def cholesky_bytes(self, panel_pairs=None, max_rank=None):
        """device bytes a `cholesky` call takes (qemb_int_cholesky_bytes): pair stage and lists, the diagonal, one panel (npair x panel) and the factor up to
        max_rank -- the figure the call checks against the free memory and the limit of qemb_int4c_mem_limit before it allocates anything"""
        from . import _lib
        b = C.c_int64()
        _lib.check(self.lib.qemb_int_cholesky_bytes(self.h, int(panel_pairs or 0), int(max_rank or 0), C.byref(b)), "qemb_int_cholesky_bytes", self.lib)
        return b.value

    def cholesky_stats(self):
        """dict(rank, panels, columns, max_d) of the last decomposition of this basis: vectors, panels, integral columns evaluated, the final largest residual diagonal"""
        from . import _lib
        out = (C.c_double * 4)()
        _lib.check(self.lib.qemb_int_cholesky_stats(self.h, out), "qemb_int_cholesky_stats", self.lib)
        return dict(rank=int(out[0]), panels=int(out[1]), columns=int(out[2]), max_d=float(out[3]))

    def free(self):
        if getattr(self, "h", None):
            self.lib.qemb_int_basis_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _symmetric_density(dm, N):
    """`dm` as a contiguous, exactly symmetric N x N array; ValueError when max |D - D^T| > 1e-12 max |D| (the direct J / K digest assumes D = D^T)"""
    dm = np.asarray(dm, dtype=float)
    if dm.shape != (N, N):
        raise ValueError(f"get_jk: the density must be {N} x {N}, not {dm.shape}")
    if np.abs(dm - dm.T).max() > 1e-12 * np.abs(dm).max():
        raise ValueError("get_jk: the density matrix is not symmetric (max |D - D^T| > 1e-12 max |D|)")
    return np.ascontiguousarray(0.5 * (dm + dm.T))


INT_LAYOUTS = {"pqL": 0, "Lpq": 1, "packed": 2, "pairs": 3}


def _int3c_hip(mol, auxmol, layout, pairs=None, lib=None):
    from . import _lib
    b, a = DeviceBasis(mol, lib), DeviceBasis(auxmol, lib)
    try:
        N, na = mol.nao, auxmol.nao
        if pairs is None:
            out = np.empty({"pqL": (N, N, na), "Lpq": (na, N, N), "packed": (na, N * (N + 1) // 2)}[layout])
            pp, n = None, 0
        else:
            pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
            out = np.empty((len(pairs), na))
            pp, n = pairs.ctypes.data, len(pairs)
        _lib.check(b.lib.qemb_int3c2e(b.h, a.h, pp, n, INT_LAYOUTS[layout], out.ctypes.data, 0), "qemb_int3c2e", b.lib)
        return out
    finally:
        b.free(); a.free()


def int2c2e(auxmol: Mole, backend="host", lib=None):
    """(P|Q), auxmol.intor('int2c2e') (molbe/eri_onthefly.py:106-108, eri_sparse_DF.py:611).  backend="hip": evaluated on the device."""
    if _backend(backend):
        from . import _lib
        a = DeviceBasis(auxmol, lib)
        try:
            out = np.empty((auxmol.nao, auxmol.nao))
            _lib.check(a.lib.qemb_int2c2e(a.h, out.ctypes.data, 0), "qemb_int2c2e", a.lib)
            return out
        finally:
            a.free()
    lib = _load()
    n = auxmol.ncart
    out = np.zeros((n, n))
    lib.gto_eri_2c(n, auxmol._arr(), out.ctypes.data_as(C.c_void_p))
    return auxmol._sph2(out)


def aux_e2(mol: Mole, auxmol: Mole, backend="host", lib=None):
    """(mu nu|P), dense (N, N, naux): pyscf.df.incore.aux_e2(mol, auxmol, 'int3c2e') (eri_onthefly.py:64-98).  backend="hip": the same array
    from the device kernels (qemb_int3c2e)."""
    if _backend(backend):
        return _int3c_hip(mol, auxmol, "pqL", lib=lib)
    lib = _load()
    out = np.zeros((mol.ncart, mol.ncart, auxmol.ncart))
    lib.gto_eri_3c(mol.ncart, mol._arr(), auxmol.ncart, auxmol._arr(), out.ctypes.data_as(C.c_void_p))
    if not auxmol.cart:
        out = out @ auxmol.c2s
    if not mol.cart:
        out = np.einsum("pqP,pi,qj->ijP", out, mol.c2s, mol.c2s, optimize=True)
    return out


def aux_e2_pairs(mol: Mole, auxmol: Mole, pairs, backend="host", lib=None):
    """(mu nu|P) for a list of AO pairs only: (npairs, naux), one auxiliary vector per pair -- the fill of the semi-sparse tensor
    (get_sparse_P_mu_nu, eri_sparse_DF.py:410-494, which asks libcint for the shell blocks that contain the reachable pairs).
    backend="hip": the shell blocks that hold the pairs are evaluated on the device."""
    if _backend(backend):
        return _int3c_hip(mol, auxmol, "pairs", pairs=pairs, lib=lib)
    lib = _load()
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if mol.cart:
        cp = pairs
        W = None
    else:
        # a spherical AO is a combination of the Cartesian functions of its shell: compute every Cartesian pair of the shell pairs touched
        sh_of = np.repeat(np.arange(mol.nbas), [2 * s[1] + 1 for s in mol.shells])
        cart_of_shell = [np.arange(s[5], s[5] + len(cart_components(s[1]))) for s in mol.shells]
        need = sorted(set((int(sh_of[p]), int(sh_of[q])) for p, q in pairs))
        cp = np.array([(a, b) for si, sj in need for a in cart_of_shell[si] for b in cart_of_shell[sj]], dtype=np.int64)
    pi = np.ascontiguousarray(cp[:, 0], dtype=np.int32); pj = np.ascontiguousarray(cp[:, 1], dtype=np.int32)
    out = np.zeros((len(cp), auxmol.ncart))
    lib.gto_eri_3c_pairs(mol.ncart, mol._arr(), auxmol.ncart, auxmol._arr(), C.c_long(len(cp)), pi.ctypes.data_as(C.c_void_p),
                         pj.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if not auxmol.cart:
        out = out @ auxmol.c2s
    if mol.cart:
        return out
    where = {(int(a), int(b)): k for k, (a, b) in enumerate(cp)}
    res = np.zeros((len(pairs), out.shape[1]))
    for k, (p, q) in enumerate(pairs):
        ca, cb = np.nonzero(mol.c2s[:, p])[0], np.nonzero(mol.c2s[:, q])[0]
        for a in ca:
            for b in cb:
                res[k] += mol.c2s[a, p] * mol.c2s[b, q] * out[where[(int(a), int(b))]]
    return res


def one_electron(mol: Mole, backend="host", lib=None):
    """(S, T, V) of `mol`.  backend="host": Mole.one_electron() (libqemb_gto); backend="hip": the device kernel (DeviceBasis.one_electron)."""
    if _backend(backend):
        b = DeviceBasis(mol, lib)
        try:
            return b.one_electron()
        finally:
            b.free()
    return mol.one_electron()


def dipole(mol: Mole, origin=(0.0, 0.0, 0.0), backend="host", lib=None):
    """The dipole integrals <a|r - origin|b> of `mol`, (3, nao, nao), origin in Bohr.  backend="host": libqemb_gto (Mole.dipole); backend="hip": the device kernel
    (DeviceBasis.dipole)."""
    if _backend(backend):
        b = DeviceBasis(mol, lib)
        try:
            return b.dipole(origin)
        finally:
            b.free()
    return mol.dipole(origin)


def pack_eri(eri_s1, sym):
    """The full [N]^4 tensor in PySCF's 4-fold ([npair][npair]) or 8-fold (1-D npair (npair + 1) / 2) packed form (pair index ij = i (i + 1) / 2 + j, i >= j)."""
    if sym == 1:
        return eri_s1
    N = eri_s1.shape[0]
    il = np.tril_indices(N)
    s4 = eri_s1[il[0], il[1]][:, il[0], il[1]]
    if sym == 4:
        return np.ascontiguousarray(s4)
    if sym == 8:
        return np.ascontiguousarray(s4[np.tril_indices(s4.shape[0])])
    raise ValueError("sym must be 1, 4 or 8")


def eri(mol: Mole, sym=1, backend="host", thresh=0.0, lib=None):
    """The four-centre AO integrals (mu nu|la si), mol.intor('int2e', aosym=...) of the reference's mean field: sym = 1 [N]^4, 4 [npair][npair], 8 1-D.
    backend="host": Mole.eri_s1() packed; backend="hip": evaluated on the device (qemb_int4c2e), with Schwarz screening when thresh > 0 (a shell quartet with
    Q_ab Q_cd < thresh is stored as zeros; the host source is never screened)."""
    if sym not in (1, 4, 8):
        raise ValueError("sym must be 1, 4 or 8")
    if _backend(backend):
        b = DeviceBasis(mol, lib)
        try:
            return b.eri(sym, thresh)
        finally:
            b.free()
    return pack_eri(mol.eri_s1(), sym)


def cholesky_eri(mol: Mole, tol=1e-8, backend="hip", span=0.01, panel_pairs=None, max_rank=None, lib=None):
    """The Cholesky vectors of the AO integrals of `mol`, (M, npair) in canonical packed order (DeviceBasis.cholesky).  The decomposition exists on the device only:
    backend="host" raises ValueError."""
    if not _backend(backend):
        raise ValueError("cholesky_eri: the decomposition runs on the device only (backend='hip')")
    b = DeviceBasis(mol, lib)
    try:
        return b.cholesky(tol, span, panel_pairs, max_rank)
    finally:
        b.free()


def get_jk(mol: Mole, dm, backend="hip", thresh=0.0, lib=None):
    """(J, K) of a symmetric density.  backend="hip": integral-direct on the device (DeviceBasis.get_jk: nothing of size N^4 is formed; thresh > 0 screens
    with the density-weighted Schwarz bound); backend="host": contracted from Mole.eri_s1(), for comparison (never screened)."""
    dm = _symmetric_density(dm, mol.nao)
    if _backend(backend):
        b = DeviceBasis(mol, lib)
        try:
            return b.get_jk(dm, thresh)
        finally:
            b.free()
    e = mol.eri_s1()
    return np.einsum("pqrs,rs->pq", e, dm, optimize=True), np.einsum("pqrs,qs->pr", e, dm, optimize=True)


class RHF:
    """Closed-shell RHF with DIIS in the AO basis (generalised eigenproblem through S^-1/2).  integral_backend="hip": `_eri` comes from the device kernels in the
    8-fold packed form (PySCF's own form of mf._eri); J and K are then contracted from the packed integrals.  direct=True (with integral_backend="hip"): direct
    SCF -- `_eri` stays None, every J and K of kernel() and get_veff() is formed integral-direct on the device (DeviceBasis.get_jk, screened at direct_thresh)
    from one DeviceBasis kept on the object; those sums are accumulated with atomic adds, so energies agree from run to run to rounding, not to the bit.
    density_fit=X (with integral_backend="hip", not with direct=True): the mean field of the fitted integrals from ONE resident 3-index tensor, exposed as
    `with_df` (eri_transform.DFContext).  X: an auxiliary-basis spec of `make_auxmol` (DFContext.from_mol), "cholesky" / ("cholesky", tol) (DFContext.from_cholesky:
    the Cholesky factor of the AO integrals, no auxiliary basis), or a ready dense DFContext, which is borrowed -- `free()` leaves it alone.  `_eri` stays None;
    S and hcore come from the device (DeviceBasis.one_electron); kernel() forms J and K from the occupied orbitals (DFContext.get_jk_orbitals), get_veff(dm) from
    any symmetric density (DFContext.get_jk).  No atomics on this route: energies repeat to the bit."""

    def __init__(self, mol: Mole, conv_tol=1e-12, max_cycle=100, integral_backend="host", lib=None, direct=False, direct_thresh=0.0, density_fit=None):
        self.integral_backend, self._lib = ("hip" if _backend(integral_backend) else "host"), lib
        self.direct, self.direct_thresh = bool(direct), float(direct_thresh)
        if self.direct and self.integral_backend != "hip":
            raise ValueError("RHF: direct=True forms J and K on the device; it needs integral_backend='hip'")
        self.density_fit, self.with_df, self._owns_df = density_fit, None, False
        if density_fit is not None:
            if self.integral_backend != "hip":
                raise ValueError("RHF: density_fit keeps the 3-index tensor on the device; it needs integral_backend='hip'")
            if self.direct:
                raise ValueError("RHF: density_fit and direct=True are two sources of J and K; choose one")
            from .eri_transform import DFContext
            if isinstance(density_fit, DFContext):
                if getattr(density_fit, "layout", None) != "dense" or density_fit.nao != mol.nao or getattr(density_fit, "h", None) is None:
                    raise ValueError("RHF: the DFContext given as density_fit must hold the dense [naux][N][N] tensor of this molecule "
                                     f"(its layout is {getattr(density_fit, 'layout', None)!r}; semi-sparse and periodic contexts are not supported)")
                self.with_df = density_fit      # borrowed
        self._basis = None
        self._pk = None
        self.mol = mol
        self.conv_tol, self.max_cycle = conv_tol, max_cycle
        self.mo_coeff = self.mo_energy = self.mo_occ = None
        self.e_tot = None
        self.converged = False
        self._eri = None
        self._S = self._h = None

    def _ensure_df(self):
        """the DF context of a density-fitted mean field, built at the first need (and again after free())"""
        if self.with_df is None:
            from .eri_transform import DFContext
            from . import _lib
            X, lib = self.density_fit, self._lib or _lib.init()
            if X == "cholesky" or (isinstance(X, tuple) and len(X) > 0 and X[0] == "cholesky"):
                self.with_df = DFContext.from_cholesky(self.mol, *(X[1:] if isinstance(X, tuple) else ()), lib=lib)
            else:
                self.with_df = DFContext.from_mol(self.mol, make_auxmol(self.mol, X), lib=lib)
            self._owns_df = True
        return self.with_df

    def get_ovlp(self):
        if self._S is None:
            S, T, V = one_electron(self.mol, "hip", self._lib) if self.density_fit is not None else self.mol.one_electron()
            self._S, self._h = S, T + V
        return self._S

    def get_hcore(self):
        self.get_ovlp()
        return self._h.copy()

    def energy_nuc(self):
        return self.mol.energy_nuc()

    def free(self):
        """release the device basis of a direct mean field (it is uploaded again when needed)"""
        b, self._basis = getattr(self, "_basis", None), None
        if b is not None:
            b.free()
        if getattr(self, "_owns_df", False) and self.with_df is not None:      # a borrowed context is the caller's
            self.with_df.free()
            self.with_df, self._owns_df = None, False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _jk(self, dm, C_occ=None):
        if self.density_fit is not None:
            df = self._ensure_df()
            return df.get_jk_orbitals(C_occ, 2.0) if C_occ is not None else df.get_jk(dm)
        if self.direct:
            if self._basis is None:
                self._basis = DeviceBasis(self.mol, self._lib)
            return self._basis.get_jk(dm, self.direct_thresh)
        e = self._eri
        if np.ndim(e) != 4:
            return self._jk_packed(dm)
        return np.einsum("pqrs,rs->pq", e, dm, optimize=True), np.einsum("pqrs,qs->pr", e, dm, optimize=True)

    def _jk_packed(self, dm):
        """J and K from `_eri` in the 4-fold or 8-fold packed form: rows over the pairs p >= q, each row unpacked to a symmetric N x N image once."""
        N = self.mol.nao
        il = np.tril_indices(N)
        npair = len(il[0])
        if self._pk is None or self._pk[0] is not self._eri:
            e = np.asarray(self._eri)
            if e.size == npair * npair:
                s4 = e.reshape(npair, npair)
            elif e.size == npair * (npair + 1) // 2:
                s4 = np.zeros((npair, npair))
                s4[np.tril_indices(npair)] = e.ravel()
                s4 = s4 + s4.T - np.diag(np.diag(s4))
            else:
                raise ValueError("RHF: `_eri` must be [N]^4, [npair][npair] or 1-D npair (npair + 1) / 2")
            rows = np.zeros((npair, N, N))
            rows[:, il[0], il[1]] = s4
            rows[:, il[1], il[0]] = s4
            self._pk = (self._eri, s4, rows)
        _, s4, rows = self._pk
        dm = np.asarray(dm)
        dp = dm[il] + dm.T[il]
        dp[il[0] == il[1]] *= 0.5
        J = np.zeros((N, N))
        J[il] = s4 @ dp
        J = J + J.T - np.diag(np.diag(J))
        K = np.zeros((N, N))
        np.add.at(K, il[0], np.einsum("xrs,xs->xr", rows, dm[il[1]]))      # K[p, r] += (pq|rs) D[q, s]
        off = il[0] != il[1]
        np.add.at(K, il[1][off], np.einsum("xrs,xs->xr", rows[off], dm[il[0][off]]))
        return J, K

    def get_veff(self, dm=None):
        dm = self.make_rdm1() if dm is None else dm
        J, K = self._jk(dm)
        return J - 0.5 * K

    def make_rdm1(self):
        no = self.mol.nelectron // 2
        return 2.0 * self.mo_coeff[:, :no] @ self.mo_coeff[:, :no].T

    def kernel(self):
        S = self.get_ovlp(); h = self._h
        if self._eri is None and not self.direct and self.density_fit is None:
            self._eri = eri(self.mol, 8, "hip", lib=self._lib) if self.integral_backend == "hip" else self.mol.eri_s1()
        no = self.mol.nelectron // 2
        w, U = np.linalg.eigh(S)
        X = U / np.sqrt(w) @ U.T
        e, c = np.linalg.eigh(X @ h @ X)
        Cm = X @ c
        dm = 2.0 * Cm[:, :no] @ Cm[:, :no].T
        # the density-fitted route forms J and K from the occupied orbitals; every other route keeps its one-argument call
        jk = (lambda d, Cm: self._jk(d, Cm[:, :no])) if self.density_fit is not None else (lambda d, Cm: self._jk(d))
        fs, es = [], []
        e_old = None
        for cyc in range(self.max_cycle):
            J, K = jk(dm, Cm)
            F = h + J - 0.5 * K
            e_el = 0.5 * np.sum((h + F) * dm)
            err = X @ (F @ dm @ S - S @ dm @ F) @ X
            if e_old is not None and abs(e_el - e_old) < self.conv_tol and np.linalg.norm(err) < 1e-8:
                self.converged = True
                break
            e_old = e_el
            fs.append(F); es.append(err); fs, es = fs[-8:], es[-8:]
            Fd = F
            if len(fs) > 1:
                m = len(fs)
                B = np.zeros((m + 1, m + 1)); B[-1, :] = B[:, -1] = 1.0; B[-1, -1] = 0.0
                for i in range(m):
                    for j in range(m):
                        B[i, j] = np.vdot(es[i], es[j])
                rhs = np.zeros(m + 1); rhs[-1] = 1.0
                try:
                    cf = np.linalg.solve(B, rhs)[:m]
                    Fd = sum(a * b for a, b in zip(cf, fs))
                except np.linalg.LinAlgError:
                    pass
            e, c = np.linalg.eigh(X @ Fd @ X)
            Cm = X @ c
            dm = 2.0 * Cm[:, :no] @ Cm[:, :no].T
        J, K = jk(dm, Cm)
        F = h + J - 0.5 * K
        e, c = np.linalg.eigh(X @ F @ X)
        self.mo_energy, self.mo_coeff = e, X @ c
        self.mo_occ = np.zeros(len(e)); self.mo_occ[:no] = 2.0
        self.e_tot = 0.5 * np.sum((h + F) * dm) + self.energy_nuc()
        return self.e_tot
