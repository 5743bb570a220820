"""LPs of general form whose unique optimal primal and dual solution is known
in closed form, at any size, and a KKT certificate for any bound types.

gen_vertex builds the LP backwards from its answer: a point x0, a basis of
exactly m of the m + n variables (rows first) that sit strictly inside their
bounds with zero dual, every other variable on a bound with a dual of the sign
optimality demands, and the costs c = A'y + d that make this point stationary.
Primal and dual non-degeneracy and a non-singular basis matrix make the
optimum unique, so a solver must return these very vectors whatever pivots it
takes.  The reference is the construction itself: it depends neither on the
GPU code nor on the oracle.

general_kkt is written from the textbook optimality conditions of

    min / max  c0 + c'x   s.t.  r = A x,  l <= (r, x) <= u

with duals (y, d), d = c - A'y: for a minimum a dual may be positive only on a
variable at its lower bound and negative only at its upper bound; for a
maximum the signs swap.  numpy only, deterministic from the seed.
"""
from __future__ import annotations

import numpy as np

from glpk_js_amd import problems
from glpk_js_amd.problems import (GLP_BS, GLP_DB, GLP_FR, GLP_FX, GLP_LO, GLP_MAX, GLP_MIN, GLP_NF, GLP_NL,
                                  GLP_NS, GLP_NU, GLP_UP)

# (m, n, dens, seeds): the sizes at which the kernels' partitioning changes;
# the two seeds of each size give one GLP_MAX and one GLP_MIN instance.  The
# oracle accompanies the instances with m <= ORACLE_MAX_M (it needs 10 - 20 s
# on one core for each of the larger ones); every instance with m <=
# ORACLE_MAX_M is admitted by tests/test_lpgen.py: the oracle alone solves it
# to the closed form.  (130 x 300: seed 6, the first GLP_MIN one, was not
# admitted: its infeasible variant is also dual infeasible, and the oracle's
# dual ends it INFEAS / NOFEAS instead of proving primal infeasibility.)
INSTANCES = (
    (70, 150, 0.6, (1, 2)),          # just past one wavefront of rows
    (130, 300, 0.6, (1, 7)),         # several waves, one 256-row group
    (270, 530, 0.6, (1, 2)),         # second row group, second 512-column tile
    (300, 700, 0.4, (1, 2)),         # nnz < 0.5 m n: A stored sparse on the explicit inverse
    (300, 1100, 0.02, (1, 4)),       # sparse A, default factor and GK_SPARSE=1
    (1030, 2100, 0.6, (1, 2)),       # MFMA panel, Newton refinement, fone / fupd limits
    (2100, 4300, 0.002, (3, 1)),     # the default factor_choice takes the sparse LU
)
ORACLE_MAX_M = 300
BAD_SCALE = (270, 530, 0.6, (1, 2))

# the shares genMix (tests/golden/gen_golden.js) draws for a feasible problem
_SHARES = ((GLP_FR, 0.08), (GLP_LO, 0.38), (GLP_UP, 0.58), (GLP_DB, 0.95), (GLP_FX, 1.0))


def _csc(a):
    """CSC arrays (0-based offsets, 1-based rows, rows ascending) of dense a."""
    m, n = a.shape
    cols, rows = np.nonzero(a.T)
    ptr = np.zeros(n + 1, np.int32)
    np.add.at(ptr, cols + 1, 1)
    return np.cumsum(ptr).astype(np.int32), (rows + 1).astype(np.int32), np.ascontiguousarray(a[rows, cols])


def _problem(a, direction, c0, c, rtype, rlb, rub, ctype, clb, cub, name):
    m, n = a.shape
    ptr, ind, val = _csc(a)
    i8 = lambda v: np.ascontiguousarray(v, np.int8)
    f8 = lambda v: np.ascontiguousarray(v, np.float64)
    return problems.Problem(
        m=m, n=n, dir=direction, c0=float(c0),
        row_type=i8(rtype), row_lb=f8(rlb), row_ub=f8(rub), rii=np.ones(m), row_stat=i8(np.full(m, GLP_BS)),
        col_type=i8(ctype), col_lb=f8(clb), col_ub=f8(cub), col_coef=f8(c), sjj=np.ones(n),
        col_stat=problems._col_stat_for(ctype, clb, cub), col_kind=i8(np.full(n, problems.GLP_CV)),
        A_ptr=ptr, A_ind=ind, A_val=val, name=name, dense=np.asfortranarray(a))


def gen_vertex(seed, m, n, dens, bad_scale=False):
    """(Problem, want): want holds the unique optimum x, r = A x, the duals y
    (rows) and d (columns), the objective z, and the optimal basis as
    row_stat / col_stat."""
    rng = np.random.default_rng([seed, m, n])
    direction = GLP_MIN if rng.random() < 0.5 else GLP_MAX
    sgn = 1.0 if direction == GLP_MIN else -1.0
    N = m + n
    # A: multiples of 1/16 in [-9, 9], a zero draw becomes 1, no empty column
    a = np.round((rng.random((m, n)) * 18.0 - 9.0) * 16.0) / 16.0
    a[a == 0.0] = 1.0
    a *= rng.random((m, n)) < dens
    for j in np.nonzero(~a.any(axis=0))[0]:
        a[rng.integers(m), j] = np.round((rng.random() * 8.0 + 1.0) * 16.0) / 16.0
    x0 = np.round((rng.random(n) * 10.0 - 5.0) * 4.0) / 4.0
    # types of the m + n variables, rows first
    t = rng.random(N)
    typ = np.full(N, GLP_FX, np.int8)
    for code, upto in reversed(_SHARES):
        typ[t < upto] = code
    # the basis: every FR variable, no FX variable, the rest at random
    basic = typ == GLP_FR
    free = np.nonzero((typ != GLP_FR) & (typ != GLP_FX))[0]
    need = m - int(basic.sum())
    assert 0 <= need <= len(free), "the seed leaves no basis of m variables"
    basic[rng.permutation(free)[:need]] = True
    brow, bcol = basic[:m], basic[m:]
    if dens < 0.1:
        # a sparse random basis matrix is singular: give A[non-basic rows,
        # basic columns] (square by construction) a transversal of large entries
        nbr, bc = np.nonzero(~brow)[0], np.nonzero(bcol)[0]
        assert len(nbr) == len(bc)
        bc = rng.permutation(bc)
        a[nbr, bc] = (8.0 + np.round(rng.random(len(bc)) * 16.0) / 16.0) * rng.choice([-1.0, 1.0], len(bc))
    rmargin = np.ones(m)
    if bad_scale:
        a = a * (2.0 ** rng.integers(-8, 9, m))[:, None] * (2.0 ** rng.integers(-8, 9, n))[None, :]
        cnt = np.maximum(1, np.count_nonzero(a, axis=1))
        rmargin = np.maximum(np.abs(a).sum(axis=1) / cnt, 2.0 ** -40)
    r0 = a @ x0
    v = np.concatenate([r0, x0])
    margin = np.concatenate([rmargin, np.ones(n)])
    w1 = (1.0 + np.round(rng.random(N) * 40.0) / 4.0) * margin
    w2 = (1.0 + np.round(rng.random(N) * 40.0) / 4.0) * margin
    at_upper = rng.random(N) < 0.5
    lb, ub = np.zeros(N), np.zeros(N)
    stat = np.full(N, GLP_BS, np.int8)
    has_lb = (typ == GLP_LO) | (typ == GLP_DB)
    has_ub = (typ == GLP_UP) | (typ == GLP_DB)
    lb[has_lb], ub[has_ub] = (v - w1)[has_lb], (v + w2)[has_ub]       # strictly inside; the basic ones keep this
    nb = ~basic
    on_lo = nb & ((typ == GLP_LO) | ((typ == GLP_DB) & ~at_upper))
    on_up = nb & ((typ == GLP_UP) | ((typ == GLP_DB) & at_upper))
    fx = typ == GLP_FX
    lb[on_lo], ub[on_up] = v[on_lo], v[on_up]
    lb[fx] = ub[fx] = v[fx]
    stat[on_lo], stat[on_up], stat[fx] = GLP_NL, GLP_NU, GLP_NS
    # duals: zero on the basis, 0.5 .. 5 with the sign of optimality elsewhere
    mag = 0.5 + np.round(rng.random(N) * 36.0) / 8.0
    dual = np.zeros(N)
    dual[on_lo], dual[on_up] = sgn * mag[on_lo], -sgn * mag[on_up]
    dual[fx] = (mag * rng.choice([-1.0, 1.0], N))[fx]
    y, d = dual[:m].copy(), dual[m:].copy()
    if bad_scale:
        y /= np.maximum(np.abs(a).max(axis=1), 2.0 ** -40)
    c = a.T @ y + d
    c0 = 1.0 + np.round(rng.random() * 100.0) / 4.0
    z = c0 + float(c @ x0)
    name = f"vertex_s{seed}_{m}x{n}_d{dens}" + ("_bad" if bad_scale else "")
    prob = _problem(a, direction, c0, c, typ[:m], lb[:m], ub[:m], typ[m:], lb[m:], ub[m:], name)
    want = dict(x=x0, r=r0, y=y, d=d, z=z, row_stat=stat[:m].copy(), col_stat=stat[m:].copy())
    return prob, want


def infeasible(prob, want):
    """The base with row 2 a copy of row 1, row 1 <= r0 and row 2 >= r0 + 3
    (r0 the base's activity of row 1 at its optimum)."""
    a = np.array(prob.dense, order="C")
    a[1] = a[0]
    rtype, rlb, rub = prob.row_type.copy(), prob.row_lb.copy(), prob.row_ub.copy()
    r0 = float(want["r"][0])
    rtype[0], rlb[0], rub[0] = GLP_UP, 0.0, r0
    rtype[1], rlb[1], rub[1] = GLP_LO, r0 + 3.0, 0.0
    return _problem(a, prob.dir, prob.c0, prob.col_coef, rtype, rlb, rub, prob.col_type, prob.col_lb, prob.col_ub,
                    prob.name + "_infeasible")


def unbounded(prob):
    """The base with the matrix entries of its first FR column cleared and
    that column's cost set to 1: a free ray in the objective."""
    fr = np.nonzero(prob.col_type == GLP_FR)[0]
    assert len(fr), "the instance has no FR column"
    a = np.array(prob.dense, order="C")
    a[:, fr[0]] = 0.0
    c = prob.col_coef.copy()
    c[fr[0]] = 1.0
    return _problem(a, prob.dir, prob.c0, c, prob.row_type, prob.row_lb, prob.row_ub, prob.col_type, prob.col_lb,
                    prob.col_ub, prob.name + "_unbounded")


def warm(prob, want):
    """A copy of prob that starts from the constructed optimal basis."""
    p = prob.copy()
    p.row_stat, p.col_stat = want["row_stat"].copy(), want["col_stat"].copy()
    return p


def solution(P):
    """The solution vectors, 0-based, of a GkProblem (1-based attributes) or
    of a result dict (the oracle's result(), a fixture's run)."""
    if isinstance(P, dict):
        g = lambda k: np.asarray(P[k])
        return dict(obj_val=float(P["obj_val"]), **{k: g(k) for k in (
            "row_stat", "col_stat", "row_prim", "col_prim", "row_dual", "col_dual")})
    return dict(obj_val=float(P.obj_val), **{k: np.asarray(getattr(P, k))[1:] for k in (
        "row_stat", "col_stat", "row_prim", "col_prim", "row_dual", "col_dual")})


def vector_errors(P, want):
    """max-abs error of each solution vector against the closed form, relative
    to 1 + max-abs of the closed form's vector"""
    s = solution(P)
    out = {}
    for key, w in (("col_prim", want["x"]), ("row_prim", want["r"]), ("row_dual", want["y"]),
                   ("col_dual", want["d"])):
        out[key] = float(np.max(np.abs(np.asarray(s[key], np.float64) - w), initial=0.0) /
                         (1.0 + np.abs(w).max(initial=0.0)))
    return out


def _matvecs(prob, x, y):
    """(A x, A'y) from the Problem's CSC arrays."""
    cols = np.repeat(np.arange(prob.n), np.diff(prob.A_ptr))
    rows = prob.A_ind - 1
    ax = np.bincount(rows, weights=prob.A_val * x[cols], minlength=prob.m)[:prob.m] if prob.m else np.zeros(0)
    aty = np.bincount(cols, weights=prob.A_val * y[rows], minlength=prob.n)[:prob.n] if prob.n else np.zeros(0)
    return ax, aty


def general_kkt(P, prob, tol=1e-7):
    """Certificate of an optimal basic solution for any bound types,
    direction and objective constant.  Returns the residuals; raises
    AssertionError on a violation.

    primal_*: every row and column inside its own bounds, tol (1 + |bound|)
    row_act: row_prim = A x;  reduced_costs: col_dual = c - A' row_dual
    dual_sign: for min a dual > 0 needs a lower bound and < 0 an upper bound
      (for max the reverse), and a basic (or NF) variable has none
    status: a non-basic variable sits on the bound its status names
    compl: dual times distance to the bound it prices is zero
    obj: obj_val = c0 + c'x (1e-9 relative)"""
    s = solution(P)
    m, n = prob.m, prob.n
    x, r = np.asarray(s["col_prim"], np.float64), np.asarray(s["row_prim"], np.float64)
    y, d = np.asarray(s["row_dual"], np.float64), np.asarray(s["col_dual"], np.float64)
    c = prob.col_coef
    ax, aty = _matvecs(prob, x, y)
    v = np.concatenate([r, x])
    dual = np.concatenate([y, d])
    typ = np.concatenate([prob.row_type, prob.col_type])
    lb = np.concatenate([prob.row_lb, prob.col_lb])
    ub = np.concatenate([prob.row_ub, prob.col_ub])
    stat = np.concatenate([s["row_stat"], s["col_stat"]])
    has_lb = np.isin(typ, (GLP_LO, GLP_DB, GLP_FX))
    has_ub = np.isin(typ, (GLP_UP, GLP_DB, GLP_FX))
    ub = np.where(typ == GLP_FX, lb, ub)
    sgn = 1.0 if prob.dir == GLP_MIN else -1.0
    cs = 1.0 + np.abs(c).max(initial=0.0)
    below = np.where(has_lb, (lb - v) / (1.0 + np.abs(lb)), 0.0)
    above = np.where(has_ub, (v - ub) / (1.0 + np.abs(ub)), 0.0)
    sd = sgn * dual / cs
    on_lo = np.where(has_lb, np.abs(v - lb) / (1.0 + np.abs(lb)), np.inf)
    on_up = np.where(has_ub, np.abs(v - ub) / (1.0 + np.abs(ub)), np.inf)
    obj = prob.c0 + float(c @ x)
    zs = 1.0 + abs(obj)
    res = {
        "primal_rows": float(max(0.0, below[:m].max(initial=0.0), above[:m].max(initial=0.0))),
        "primal_cols": float(max(0.0, below[m:].max(initial=0.0), above[m:].max(initial=0.0))),
        "row_act": float(np.abs(ax - r).max(initial=0.0) / (1.0 + np.abs(ax).max(initial=0.0))),
        "reduced_costs": float(np.abs((c - aty) - d).max(initial=0.0) / cs),
        # a dual of the wrong sign for the bounds the variable has
        "dual_sign": float(max(0.0, np.where(has_lb, 0.0, sd).max(initial=0.0),
                               np.where(has_ub, 0.0, -sd).max(initial=0.0))),
        "dual_basic": float(np.abs(sd[(stat == GLP_BS) | (stat == GLP_NF)]).max(initial=0.0)),
        "dual_at_lower": float(max(0.0, (-sd[stat == GLP_NL]).max(initial=0.0))),
        "dual_at_upper": float(max(0.0, sd[stat == GLP_NU].max(initial=0.0))),
        "status_lower": float(on_lo[(stat == GLP_NL) | (stat == GLP_NS)].max(initial=0.0)),
        "status_upper": float(on_up[stat == GLP_NU].max(initial=0.0)),
        "compl_lower": float((np.maximum(sgn * dual, 0.0) * np.where(has_lb, np.abs(v - lb), 0.0)).max(initial=0.0)
                             / zs),
        "compl_upper": float((np.maximum(-sgn * dual, 0.0) * np.where(has_ub, np.abs(ub - v), 0.0)).max(initial=0.0)
                             / zs),
        "obj": abs(obj - s["obj_val"]) / max(1.0, abs(obj)),
    }
    bad_nf = (stat == GLP_NF) & (typ != GLP_FR)
    assert not bad_nf.any(), ("NF status on a bounded variable", np.nonzero(bad_nf)[0][:5])
    for k, val in res.items():
        assert val <= (1e-9 if k == "obj" else tol), (k, val, res)
    return res
