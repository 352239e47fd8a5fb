"""NumPy / Python-integer twin of the screened Epstein-Nesbet second-order correction behind DeviceFragment.sci_pt2 (test infrastructure), on tests/sci_numpy.py.

For a selected space V with vector c and energy e_var, and a threshold eps_pt > 0 (DESIGN.md §4 "Selected CI"):
  S_a   = sum over i in V with |H_ai c_i| >= eps_pt of H_ai c_i      (a outside V; each product tested on its own, as in the selection rule)
  E_PT2 = sum_a S_a^2 / (e_var - H_aa)                               (denominators not guarded)
over every a outside V with at least one passing product and its spin-swapped partner (a partner without a passing product has S = 0 and adds nothing, but
counts in n_ext).  Source-driven: for every member i and every connected a outside V the product is added to a dict when it passes -- the other way round from
the device's row pass, which walks the space for every external.  margin = min | |H_ai c_i| / eps_pt - 1 | over the non-zero products: how far the nearest
decision was from the threshold."""
import numpy as np

import sci_numpy as snp


def _finish(S, e_var, margin, diag, products):
    keys = sorted(S)
    contrib = np.array([S[a] ** 2 / (e_var - diag(a)) for a in keys])
    return dict(e_pt2=float(contrib.sum()), n_ext=len(keys), abs_sum=float(np.abs(contrib).sum()), margin=float(margin), products=products, keys=keys,
                contrib=contrib)


def pt2(h, V, n, dets, c, e_var, eps_pt):
    """dict(e_pt2, n_ext, abs_sum = sum |contribution|, margin, products = how many products passed, keys, contrib) by the rules on Python integers"""
    inside = set(dets)
    S, margin, products = {}, np.inf, 0
    for d, ci in zip(dets, c):
        if ci == 0.0:
            continue
        for a in snp.connected(d, n):
            if a in inside:
                continue
            x = snp.hij(h, V, a, d) * ci
            if x != 0.0:
                margin = min(margin, abs(abs(x) / eps_pt - 1.0))
            if abs(x) >= eps_pt:
                products += 1
                S[a] = S.get(a, 0.0) + x
                if (a[1], a[0]) not in inside:
                    S.setdefault((a[1], a[0]), 0.0)
    return _finish(S, e_var, margin, lambda a: snp.hij(h, V, a, a), products)


def pt2_many(h, V, n, dets, c, e_var, eps_pt):
    """`pt2` with the rules evaluated on arrays (snp.hij_many, snp._targets): thousands of determinants with wide words.  Every excitation of every member is
    evaluated -- no shortcut by a bound on the elements."""
    inside = set(dets)
    S, margin, products = {}, np.inf, 0
    for d, ci in zip(dets, c):
        if ci == 0.0:
            continue
        sa, da = snp._targets(d[0], n)
        sb, db = snp._targets(d[1], n)
        A, B = np.uint64(d[0]), np.uint64(d[1])
        ta = np.concatenate([sa, np.full(sb.shape, A), da, np.full(db.shape, A), np.repeat(sa, len(sb))])
        tb = np.concatenate([np.full(sa.shape, B), sb, np.full(da.shape, B), db, np.tile(sb, len(sa))])
        x = snp.hij_many(h, V, ta, tb, np.full(ta.shape, A), np.full(ta.shape, B)) * ci
        near = np.abs(np.abs(x) / eps_pt - 1.0)
        near[x == 0.0] = np.inf
        for k in np.argsort(near):      # the nearest decision about a determinant outside the space
            if not near[k] < margin:
                break
            if (int(ta[k]), int(tb[k])) not in inside:
                margin = float(near[k])
                break
        for k in np.nonzero(np.abs(x) >= eps_pt)[0]:
            a = (int(ta[k]), int(tb[k]))
            if a in inside:
                continue
            products += 1
            S[a] = S.get(a, 0.0) + float(x[k])
            if (a[1], a[0]) not in inside:
                S.setdefault((a[1], a[0]), 0.0)
    keys = sorted(S)
    ka, kb = np.array([a[0] for a in keys], dtype=np.uint64), np.array([a[1] for a in keys], dtype=np.uint64)
    diag = dict(zip(keys, snp.hij_many(h, V, ka, kb, ka, kb)))
    return _finish(S, e_var, margin, lambda a: diag[a], products)
