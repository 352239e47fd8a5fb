"""Shared cases of the DF-integral tests (test_gpu_int3c.py on the device, test_int3c_hostlogic.py through the scalar twin): every check takes the
library handle, so the same comparison against the host integral source runs on both."""
import ctypes as C

import numpy as np

from quemb_amd import _lib
from quemb_amd import integrals as I

BAR = 1e-10                      # max |dev - host| <= BAR * max(1, max |host|): ten times inside the 1e-9 of the DF transform comparisons
BOYS_SWITCH = 35.0               # series below, asymptotic form from here on (int3c_core.h)
BOYS_POINTS = [0.0, 1e-12, 1e-6, 0.1, 1.0, 5.0, 15.0, 25.0, 30.0, 35.0, 60.0, 200.0, BOYS_SWITCH * (1 - 1e-9), BOYS_SWITCH * (1 + 1e-9), 34.5, 35.5]

# 2-3 primitives per shell, exponents of ordinary valence / fitting functions
_EXP = {0: ([2.3, 0.7, 0.25], [0.3, 0.5, 0.4]), 1: ([1.6, 0.45], [0.55, 0.6]), 2: ([1.2, 0.5, 0.3], [0.4, 0.5, 0.3]), 3: ([1.4, 0.6], [0.6, 0.5]),
        4: ([1.1, 0.55], [0.5, 0.6])}
GEOMETRIES = {      # centres of shell a, shell b, auxiliary shell (Bohr): distinct, non-collinear, off the axes; one atom; a = b != P
    "three": ((0.13, -0.21, 0.32), (0.94, 0.55, -0.47), (-0.38, 0.81, 0.66)),
    "one": ((0.13, -0.21, 0.32),) * 3,
    "ab": ((0.13, -0.21, 0.32), (0.13, -0.21, 0.32), (-0.38, 0.81, 0.66)),
}
CLASSES = [(la, lb, lp) for lb in range(3) for la in range(lb + 1) for lp in range(5)]


def close(dev, host):
    d = float(np.abs(np.asarray(dev) - np.asarray(host)).max()) if np.size(host) else 0.0
    return d, d <= BAR * max(1.0, float(np.abs(host).max()) if np.size(host) else 0.0)


def boys_reference(xs, m_max=8):
    from scipy import special as sp
    m = np.arange(m_max + 1)
    ref = np.empty((len(xs), m_max + 1))
    for i, x in enumerate(xs):
        ref[i] = 1.0 / (2 * m + 1) if x == 0 else 0.5 * x ** -(m + 0.5) * sp.gamma(m + 0.5) * sp.gammainc(m + 0.5, x)
    return ref


def check_boys(lib, on_device):
    xs = np.concatenate([BOYS_POINTS, np.random.default_rng(20261017).uniform(0.0, 60.0, 200)])
    out = np.empty((len(xs), 9))
    if on_device:
        dx = _lib.DeviceBuffer.from_numpy(xs, lib=lib); do = _lib.DeviceBuffer(out.size, lib=lib)
        _lib.check(lib.qemb_op_boys(8, len(xs), dx.ptr, do.ptr), "qemb_op_boys", lib)
        out = do.numpy(out.shape)
        dx.free(); do.free()
    else:
        _lib.check(lib.qemb_op_boys(8, len(xs), xs.ctypes.data, out.ctypes.data), "qemb_op_boys", lib)
    rel = np.abs(out / boys_reference(xs) - 1.0)
    print(f"boys: max relative deviation {rel.max():.2e} at x = {xs[np.unravel_index(rel.argmax(), rel.shape)[0]]!r}")
    assert rel.max() <= 1e-13, rel.max(axis=1)
    assert (out[0] == 1.0 / (2 * np.arange(9) + 1)).all()


def class_block(lib, la, lb, lp, geom):
    """(device block, host block) of one angular class on explicit shells."""
    ra, rb, rp = GEOMETRIES[geom]
    mol = I.Mole([("H", ra), ("C", rb)], basis={"H": [(la, *_EXP[la])], "C": [(lb, *_EXP[lb])]}, unit="Bohr")
    aux = I.Mole([("H", rp)], basis={"H": [(lp, *_EXP[lp])]}, unit="Bohr")
    na, nb, npp = 2 * la + 1, 2 * lb + 1, 2 * lp + 1
    host = I.aux_e2(mol, aux)[:na, na:, :]
    out = np.empty((na, nb, npp))
    rec = [mol.bfs[mol.shells[0][5]], mol.bfs[mol.shells[1][5]], aux.bfs[0]]
    tab = I.c2s_table()
    _lib.check(lib.qemb_op_int3c_class(la, lb, lp, C.addressof(rec[0]), C.addressof(rec[1]), C.addressof(rec[2]), tab.ctypes.data, out.ctypes.data),
               "qemb_op_int3c_class", lib)
    return out, host


def check_class(lib, la, lb, lp):
    for geom in GEOMETRIES:
        dev, host = class_block(lib, la, lb, lp, geom)
        d, ok = close(dev, host)
        print(f"class ({la},{lb}|{lp}) {geom}: max |dev - host| = {d:.2e}, max |host| = {np.abs(host).max():.3e}")
        assert ok, (la, lb, lp, geom, d)
        assert np.abs(host).max() > 0 or geom == "one"      # (on one centre most classes vanish by parity: the zeros must come out as zeros too)


def h8(basis="sto-3g", n=8):
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(n)], basis=basis)
    return mol, I.make_auxmol(mol, "etb")


def octane12():
    from helpers import GOLDEN
    mol = I.Mole(I.read_xyz(GOLDEN / "octane.xyz")[:12])
    return mol, I.make_auxmol(mol, "etb")


def check_molecule(lib, mol, aux, name):
    host3, host2 = I.aux_e2(mol, aux), I.int2c2e(aux)
    dev3, dev2 = I.aux_e2(mol, aux, backend="hip", lib=lib), I.int2c2e(aux, backend="hip", lib=lib)
    d3, ok3 = close(dev3, host3); d2, ok2 = close(dev2, host2)
    print(f"{name}: N = {mol.nao}, naux = {aux.nao}, aux l up to {max(s[1] for s in aux.shells)}: (mu nu|P) {d3:.2e}, (P|Q) {d2:.2e}")
    assert ok3 and ok2, (d3, d2)
    assert (dev3 == dev3.transpose(1, 0, 2)).all() and (dev2 == dev2.T).all()                       # the mirror is a copy
    again3, again2 = I.aux_e2(mol, aux, backend="hip", lib=lib), I.int2c2e(aux, backend="hip", lib=lib)
    assert again3.tobytes() == dev3.tobytes() and again2.tobytes() == dev2.tobytes()               # every element written once: the same bits
    return host3, host2


def check_pair_list(lib):
    """The stored pairs of the H8 semi-sparse case (H8 / cc-pVDZ, N = 40, so that shells hold several functions and a pair inside one shell can be
    off-diagonal; AO screening at 1e-2 so that the list is a proper subset of the triangle), plus explicit corner pairs."""
    from quemb_amd import eri_sparse_DF as sdf
    mol, aux = h8("cc-pvdz", 8)
    assert mol.natm == 8 and mol.nao == 40
    S_abs = sdf.approx_S_abs(mol, lib=lib)
    t = sdf.get_sparse_P_mu_nu(mol, aux, sdf._get_AO_per_AO(S_abs, 1e-2, None, lib=lib), fill=False)
    pairs = sorted(((mu, nu) for mu, r in enumerate(t.exch_reachable_unique) for nu in r), key=lambda pq: t.offsets[(pq[0] * (pq[0] + 1)) // 2 + pq[1]])
    assert 0 < len(pairs) < mol.nao * (mol.nao + 1) // 2, "the list must be screened"
    last = (mol.nao - 1, mol.nao - 1)
    inside = (mol.nao - 1, mol.nao - 3)                       # two different p functions of the last shell
    assert last in pairs
    pairs = pairs + [inside, (2, 9), (9, 2)] if inside not in pairs else pairs + [(2, 9), (9, 2)]
    host = I.aux_e2_pairs(mol, aux, pairs)
    dev = I.aux_e2_pairs(mol, aux, pairs, backend="hip", lib=lib)
    d, ok = close(dev, host)
    print(f"pair list: {len(pairs)} pairs of {mol.nao * (mol.nao + 1) // 2}, max |dev - host| = {d:.2e}")
    assert ok, d
    assert (dev[-1] == dev[-2]).all()


def check_inplace_fill(lib, mol, aux, alloc_stats):
    from quemb_amd import eri_transform as et
    rng = np.random.default_rng(7)
    TA = np.linalg.qr(rng.standard_normal((mol.nao, mol.nao)))[0][:, : min(6, mol.nao)]
    df_h = et.DFContext(j2c=I.int2c2e(aux), lib=lib)
    df_h.set_ints(I.aux_e2(mol, aux), mol.nao, "pqL")
    ref = df_h.transform(TA)
    df_h.free()
    df = et.DFContext.empty(lib=lib)
    if alloc_stats:
        n, nf, ms, gb = C.c_longlong(), C.c_longlong(), C.c_double(), C.c_double()
        lib.qemb_trim_all()
        lib.qemb_alloc_stats(C.byref(n), C.byref(nf), C.byref(ms), C.byref(gb), 1)
    df.set_ints_from_mol(mol, aux)
    if alloc_stats:
        lib.qemb_alloc_stats(C.byref(n), C.byref(nf), C.byref(ms), C.byref(gb), 0)
        tensor = 8.0 * aux.nao * mol.nao * mol.nao
        got = gb.value * 1e9                                   # qemb_alloc_stats reports bytes * 1e-9
        # what a fill without staging allocates: the tensor, three naux^2 images (the metric that becomes its factor, the inverse, the work space of the
        # inversion), the shells and index lists (256 KiB is generous for them) and 25 % of the tensor for the allocator's rounding.  A staging copy of
        # the tensor would add `tensor` bytes: 2 x tensor + the rest, well above the bound when the tensor dominates the naux^2 terms (both figures are printed)
        bound = 1.25 * tensor + 8.0 * 3 * aux.nao ** 2 + 2 ** 18
        print(f"in-place fill: {got:.0f} bytes allocated for a tensor of {tensor:.0f}, bound {bound:.0f}, with a staging copy at least {2 * tensor + 8.0 * 3 * aux.nao ** 2:.0f}")
        assert got <= bound
    out = df.transform(TA)
    df.free()
    rel = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"in-place fill: transform deviates by {rel:.2e} relative")
    assert rel <= 1e-9


def be_energies(lib, int_transform, solver, integral_backend, **kw):
    from helpers import GOLDEN
    from quemb_amd.fragpart import FragPart
    from quemb_amd.mbe import BE
    mol = I.Mole([["H", (0.0, 0.0, float(i))] for i in range(8)])
    mf = be_energies.mf = getattr(be_energies, "mf", None) or I.RHF(mol)
    if mf.e_tot is None:
        mf.kernel()
    fobj = FragPart.from_json(GOLDEN / "fragmentation.json", "test_autogen_h_linear_be2")
    be = BE(mf, fobj, lib=lib, distribute=False, int_transform=int_transform, auxbasis="etb", integral_backend=integral_backend, **kw)
    e, comp = be.oneshot(solver=solver)[:2]
    return np.array([e, *comp])


def check_end_to_end(lib, int_transform, solver, **kw):
    host = be_energies(lib, int_transform, solver, "host", **kw)
    dev = be_energies(lib, int_transform, solver, "hip", **kw)
    print(f"{int_transform} {solver}: E_corr host {host[0]:.12f} hip {dev[0]:.12f}, pieces differ by {np.abs(host - dev).max():.2e}")
    assert np.abs(host - dev).max() <= 1e-9, (host, dev)
