"""Golden blocks for the DF integrals (mu nu|P) and (P|Q): tests/golden/int3c_ref.npz.

Every block is computed by the quadrature reference of tests/int3c_reference.py (no Boys function, no Hermite coefficients, no R table), at two
quadrature orders that have to agree to 1e-13 of the block's largest element, and has to hold an element of at least 1e-8 (int3c_cases.MIN_BLOCK), so
that a bar relative to the block means something.  The file holds the case definitions (shell l, exponents, coefficients, centres; JSON under "cases"),
one "ref/<name>" block per case, the worst deviation of the host source csrc_host/gto_ints.c per family ("hostdev/<family>", also printed) and the
H3 / cc-pVDZ blocks of int3c_cases.h3_layout_case ("h3/ref": lower triangle of AO pairs x naux; "h3/blocks": the shell triples kept).

Cases: one shell per role, so one block each.
  class    all 45 classes (l_a <= 2, l_b <= l_a | l_P <= 4) in both shell orders (the 45 ordered triples l_a, l_b <= 2) and the 25 metric classes (l_0 | l_1): 70 blocks, ordinary exponents,
           geometry "three" of int3c_cases
  far      the auxiliary centre 13 Bohr away (x >= 35 for most primitive triples), closer only where the block would fall below 1e-8
  switch   one primitive per shell, the auxiliary centre placed so that T = rho |P - C|^2 is 35 (1 -+ 1e-9), 34.5, 35.5
  T1e3, T1e4   a tight exponent pair (40, 25 | 30) 0.15 Bohr apart plus distance; T is lowered from the family's target until the block reaches 1e-8
           (a (d d|g) block falls like T^-2.5, a (g|g) block like T^-4.5: the T actually used is stored with the case; T1e4 keeps only the classes that
           reach 1e-8 above T = 1e3).  Where the two quadrature orders differ by more than 1e-13 -- far (d d|g) and (g|g) blocks, 1e-5 of the Cartesian
           integrals they are formed from -- the block is evaluated in mpmath instead ("certified": "mpmath"), never moved for that reason
  tight8   the eight cc-pVDZ carbon s exponents 6665 ... 0.5215 (with their contraction coefficients, typed in below) on shell a and on the
           auxiliary shell, at the l of the class: near ("three"), far and on one centre
  diffuse  exponents 0.015 - 0.03
  prim8    8 primitives on all three shells
  one, ab  the coincidences of int3c_cases.GEOMETRIES
The stress families run for the classes SPREAD3 / SPREAD2.  Single primitives of the hardest families are also evaluated in mpmath at 30 digits.

    python tests/golden/make_golden_int3c_ref.py          (a few minutes)
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import int3c_cases as cases  # noqa: E402
import int3c_reference as R  # noqa: E402

SPREAD3 = [(0, 0, 0), (1, 0, 1), (2, 1, 3), (2, 2, 4), (1, 2, 2)]
SPREAD2 = [(4, 4), (2, 1)]
DIR = np.array([0.48, -0.6, 0.64])                      # unit vector off every axis and plane
RA, RB, RP = (np.array(r) for r in cases.GEOMETRIES["three"])
MARGIN = 3.0                                            # the host block that places a far centre has to reach MARGIN * MIN_BLOCK
# cc-pVDZ carbon, the 8-primitive s contraction (Dunning 1989; EMSL basis set exchange)
C_S_EX = [6665.0, 1000.0, 228.0, 64.71, 21.06, 7.495, 2.797, 0.5215]
C_S_CO = [0.000692, 0.005329, 0.027077, 0.101718, 0.27474, 0.448564, 0.285074, 0.015204]
PRIM8 = {"a": ([0.15 * 1.9 ** k for k in range(8)], [0.3, 0.5, 0.4, -0.2, 0.35, 0.25, 0.15, 0.1]),
         "b": ([0.2 * 1.8 ** k for k in range(8)], [0.45, 0.3, 0.5, 0.2, -0.15, 0.3, 0.1, 0.05]),
         "p": ([0.12 * 2.0 ** k for k in range(8)], [0.5, 0.4, 0.3, 0.3, 0.2, -0.1, 0.1, 0.05])}
DIFFUSE = {"a": ([0.03, 0.015], [0.6, 0.5]), "b": ([0.02], [1.0]), "p": ([0.025, 0.015], [0.5, 0.6])}


def shell(l, ex, co, r):
    return {"l": int(l), "ex": [float(x) for x in ex], "co": [float(x) for x in co], "r": [float(x) for x in r]}


def make(name, family, ls, sh, **extra):
    """ls: (la, lb, lp) or (l0, l1); sh: role -> (exponents, coefficients, centre)."""
    if len(ls) == 2:
        c = {"name": name, "family": family, "kind": "2c", "a": shell(ls[0], *sh["a"]), "p": shell(ls[1], *sh["p"])}
    else:
        c = {"name": name, "family": family, "kind": "3c", "a": shell(ls[0], *sh["a"]), "b": shell(ls[1], *sh["b"]), "p": shell(ls[2], *sh["p"])}
    c.update(extra)
    return c


def tag(ls):
    return ("%d%d_%d" % ls) if len(ls) == 3 else ("m%d_%d" % ls)


def roles(ls):
    return dict(zip("abp", ls)) if len(ls) == 3 else {"a": ls[0], "p": ls[1]}


def ordinary(ls, geom):
    ra, rb, rp = cases.GEOMETRIES[geom]
    return {k: (*cases._EXP[l], r) for (k, l), r in zip(roles(ls).items(), (ra, rb, rp) if len(ls) == 3 else (ra, rp))}


def product_centre(c):
    if c["kind"] == "2c":
        return np.array(c["a"]["r"]), c["a"]["ex"][0]
    a, b = c["a"]["ex"][0], c["b"]["ex"][0]
    return (a * np.array(c["a"]["r"]) + b * np.array(c["b"]["r"])) / (a + b), a + b


def host_top(c):
    return float(np.abs(cases.case_block(c)).max())


def placed(build, trials, what):
    """The first of `trials` (distances or T values, far to near) whose HOST block reaches MARGIN * MIN_BLOCK (the reference asserts MIN_BLOCK later) and
    on which the two quadrature orders of the reference agree: a far (d d|g) or (g|g) block is what is left of Cartesian integrals 10^5 times larger,
    and below about 1e-7 even extended precision does not certify it to 1e-13."""
    for v in trials:
        c = build(v)
        if host_top(c) < MARGIN * cases.MIN_BLOCK:
            continue
        try:
            c["_ref"] = reference_block(c)
            return c
        except ArithmeticError as e:
            if all(len(c[k]["ex"]) == 1 for k in "abp" if k in c):
                # single primitives: the block is certified in mpmath at 30 digits instead (Cartesian -> spherical step included) and that value is stored;
                # the extended-precision quadrature has to agree with it to a hundredth of the bar of the tests
                m = cases.case_moles(c)
                ref = R.block_mp(None, m[0], 0, None, 1) if c["kind"] == "2c" else R.block_mp(m[0], m[1], 0, 1, 0)
                fn, args = (R.block2c, (m[0], 0, 1)) if c["kind"] == "2c" else (R.block3c, (m[0], m[1], 0, 1, 0))
                sd = cases.rel_dev(fn(*args), ref)
                print(f"{c['name']} at {v:g}: {e}; certified in mpmath, the quadrature deviates from it by {sd:.1e}", flush=True)
                assert sd <= 0.01 * cases.BAR_REL, (c["name"], sd)
                c["_ref"], c["certified"] = (ref, sd), "mpmath"
                return c
            print(f"{c['name']} at {v:g} rejected: {e}", flush=True)
    raise AssertionError(f"{what}: no placement reaches {cases.MIN_BLOCK}")


def build_cases():
    out = []
    for ls in [(la, lb, lp) for la in range(3) for lb in range(3) for lp in range(5)] + [(l0, l1) for l0 in range(5) for l1 in range(5)]:
        out.append(make("class_" + tag(ls), "class", ls, ordinary(ls, "three")))
    for ls in SPREAD3 + SPREAD2:
        def far(Rd, ls=ls):
            sh = ordinary(ls, "three")
            sh["p"] = (*sh["p"][:2], RA + Rd * DIR)
            return make("far_" + tag(ls), "far", ls, sh, distance=Rd)
        out.append(placed(far, [13.0, 11.0, 9.0, 7.0, 5.0, 3.0], "far " + tag(ls)))
        for label, T in (("below", 35.0 * (1 - 1e-9)), ("above", 35.0 * (1 + 1e-9)), ("34.5", 34.5), ("35.5", 35.5)):
            sh = {k: ([e], [1.0], r) for k, e, r in (("a", 0.9, RA), ("b", 0.6, RB), ("p", 0.7, RP))}
            c = make(f"switch_{label}_" + tag(ls), "switch", ls, sh, T=T)
            Pc, p = product_centre(c)
            c["p"]["r"] = [float(x) for x in Pc + np.sqrt(T * (p + 0.7) / (p * 0.7)) * DIR]
            out.append(c)
        for fam, targets in (("T1e3", [1e3, 300.0, 100.0, 50.0]), ("T1e4", [1e4, 3e3, 1e3, 300.0, 100.0, 50.0])):
            def tight(T, ls=ls, fam=fam):
                sh = {k: ([e], [1.0], r) for k, e, r in (("a", 40.0, RA), ("b", 25.0, RA + np.array([0.1, 0.05, -0.08])), ("p", 30.0, RP))}
                c = make(f"{fam}_" + tag(ls), fam, ls, sh, T=T)
                Pc, p = product_centre(c)
                c["p"]["r"] = [float(x) for x in Pc + np.sqrt(T * (p + 30.0) / (p * 30.0)) * DIR]
                return c
            c = placed(tight, targets, fam + " " + tag(ls))
            if fam == "T1e4" and c["T"] <= 1e3:
                continue                                 # no larger T reaches 1e-8 for this class: it would repeat the T1e3 case
            out.append(c)
        for where in ("near", "far", "one"):
            def t8(Rd, ls=ls, where=where):
                sh = ordinary(ls, "one" if where == "one" else "three")
                sh["a"] = (C_S_EX, C_S_CO, sh["a"][2]); sh["p"] = (C_S_EX, C_S_CO, sh["p"][2] if Rd is None else RA + Rd * DIR)
                return make(f"tight8_{where}_" + tag(ls), "tight8", ls, sh)
            if where == "one" and ls in ((1, 2, 2), (2, 1)):
                continue                                 # vanish by parity on one centre
            out.append(placed(t8, [11.0, 9.0, 7.0, 5.0, 3.0], "tight8 far " + tag(ls)) if where == "far" else t8(None))
        sh = ordinary(ls, "three")
        out.append(make("diffuse_" + tag(ls), "diffuse", ls, {k: (*DIFFUSE[k], sh[k][2]) for k in sh}))
        out.append(make("prim8_" + tag(ls), "prim8", ls, {k: (*PRIM8[k], sh[k][2]) for k in sh}))
        out.append(make("ab_" + tag(ls), "ab", ls, ordinary(ls, "ab")))
        if ls not in ((1, 2, 2), (2, 1)):
            out.append(make("one_" + tag(ls), "one", ls, ordinary(ls, "one")))
    assert len({c["name"] for c in out}) == len(out)
    return out


def reference_block(c, prim=None):
    m = cases.case_moles(c)
    fn, args = (R.block2c, (m[0], 0, 1)) if c["kind"] == "2c" else (R.block3c, (m[0], m[1], 0, 1, 0))
    if prim is not None:
        return fn(*args, prim=prim), 0.0
    return R.converged_block(fn, *args)


def main():
    t0 = time.time()
    all_cases = build_cases()
    out, hostdev, selfdev, mpdev = {}, {}, {}, 0.0
    for c in all_cases:
        ref, sd = c.pop("_ref", None) or reference_block(c)
        top = float(np.abs(ref).max())
        assert top >= cases.MIN_BLOCK, (c["name"], top)
        hd = cases.rel_dev(cases.case_block(c), ref)
        hostdev[c["family"]] = max(hostdev.get(c["family"], 0.0), hd); selfdev[c["family"]] = max(selfdev.get(c["family"], 0.0), sd)
        line = f"{c['name']:24s} max |ref| {top:.3e}  orders differ {sd:.1e}  host deviates {hd:.1e}" + "".join(f"  {k} = {c[k]:g}" for k in ("T", "distance") if k in c)
        nprim = int(np.prod([len(c[k]["ex"]) for k in "abp" if k in c]))
        if c["family"] in ("far", "switch", "T1e3", "T1e4") and sum(c[k]["l"] for k in "abp" if k in c) <= 2 and nprim <= 27:
            md = cases.rel_dev(reference_block(c, prim=R.primitive_mp)[0], ref)       # mpmath, 30 digits
            assert md <= R.SELF_CHECK, (c["name"], md)
            mpdev = max(mpdev, md)
            line += f"  mpmath deviates {md:.1e}"
        print(line, flush=True)
        out["ref/" + c["name"]] = ref
    # H3 / cc-pVDZ: every block whose host value reaches MARGIN * MIN_BLOCK
    mol, aux = cases.h3_layout_case()
    from quemb_amd import integrals as I
    host = I.aux_e2(mol, aux)
    il = np.tril_indices(mol.nao)
    ref3 = np.zeros((len(il[0]), aux.nao))
    lo, la = mol.ao_loc_nr(), aux.ao_loc_nr()
    where = {(int(p), int(q)): n for n, (p, q) in enumerate(zip(*il))}
    blocks, h3dev = [], 0.0
    for i in range(mol.nbas):
        for j in range(i + 1):
            for k in range(aux.nbas):
                if np.abs(host[lo[i]: lo[i + 1], lo[j]: lo[j + 1], la[k]: la[k + 1]]).max() < MARGIN * cases.MIN_BLOCK:
                    continue
                blk, sd = R.converged_block(R.block3c, mol, aux, i, j, k)
                assert np.abs(blk).max() >= cases.MIN_BLOCK
                h3dev = max(h3dev, cases.rel_dev(host[lo[i]: lo[i + 1], lo[j]: lo[j + 1], la[k]: la[k + 1]], blk))
                for x in range(blk.shape[0]):
                    for y in range(blk.shape[1]):
                        if lo[i] + x >= lo[j] + y:
                            ref3[where[(lo[i] + x, lo[j] + y)], la[k]: la[k + 1]] = blk[x, y]
                blocks.append((i, j, k))
    hostdev["h3"] = h3dev
    print(f"H3 / cc-pVDZ: {len(blocks)} of {mol.nbas * (mol.nbas + 1) // 2 * aux.nbas} blocks kept, host deviates {h3dev:.1e}")
    out["h3/ref"], out["h3/blocks"] = ref3, np.array(blocks, dtype=np.int32)
    for fam in sorted(hostdev):
        print(f"family {fam:8s}: host source deviates by at most {hostdev[fam]:.2e} of a block's largest element (orders differ by {selfdev.get(fam, 0.0):.1e})")
        out["hostdev/" + fam] = np.float64(hostdev[fam])
    print(f"mpmath (30 digits) deviates from the reference by at most {mpdev:.1e}")
    out["cases"] = np.array(json.dumps(all_cases))
    np.savez_compressed(HERE / "int3c_ref.npz", **out)
    print("wrote", HERE / "int3c_ref.npz", (HERE / "int3c_ref.npz").stat().st_size, "bytes,", len(all_cases), "cases,", f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
