"""General-bound, scaled and non-default-option LPs at multi-block sizes.

The reference is a closed form (tests/lpgen.py): LPs built backwards from a
unique non-degenerate optimal vertex, with free, lower-, upper-, double-bounded
and fixed rows and columns, both directions and a non-zero objective constant.
Whatever pivots the solver takes it must return the constructed x, A x, row
duals and reduced costs, so a kernel that prices badly, mishandles a bound
flip or signs a dual wrongly for GLP_MIN or an upper-bounded row fails here
even where the objective alone would pass.  The sizes are those at which the
kernels' partitioning changes (lpgen.INSTANCES).  Up to 300 rows the oracle
runs beside the GPU (tests/test_lpgen.py admits these instances on the CPU);
the larger ones rest on the closed form alone.

Bar: objective 1e-9 relative; vectors 1e-9 (1 + max-abs of the reference
vector) on well-scaled instances (the oracle's own error there is <= 6e-12);
on the bad_scale instances max(1e-9, 10 x the oracle's own error on that
instance), the factor 10 for a different but equally valid pivot path."""
import functools

import numpy as np
import pytest

import lpgen
from glpk_js_amd import gk, problems

pytestmark = pytest.mark.gpu

FEAS = problems.GLP_FEAS
METHODS = [pytest.param(gk.GLP_PRIMAL, id="primal"), pytest.param(gk.GLP_DUALP, id="dualp"),
           pytest.param(gk.GLP_DUAL, id="dual")]


def _cases(pick):
    return [pytest.param(m, n, dens, seed, id=f"{m}x{n}-s{seed}")
            for (m, n, dens, seeds) in lpgen.INSTANCES if pick(m, n) for seed in seeds]


SMALL = _cases(lambda m, n: m <= lpgen.ORACLE_MAX_M)
MID = _cases(lambda m, n: (m, n) in ((130, 300), (270, 530)))
VARIANT_SIZES = _cases(lambda m, n: (m, n) in ((130, 300), (300, 700)))
SPARSE_A = _cases(lambda m, n: (m, n) == (300, 1100))
PANEL = _cases(lambda m, n: m == 1030)
SPARSE_LU = _cases(lambda m, n: m == 2100)
STOPPED = _cases(lambda m, n: (m, n) == (270, 530))


@functools.lru_cache(maxsize=None)
def _instance(seed, m, n, dens, bad_scale=False):
    return lpgen.gen_vertex(seed, m, n, dens, bad_scale)


@functools.lru_cache(maxsize=None)
def _variant(seed, m, n, dens, kind):
    prob, want = _instance(seed, m, n, dens)
    return lpgen.infeasible(prob, want) if kind == "infeasible" else lpgen.unbounded(prob)


def _oracle_run(oracle, prob, **opts):
    o = oracle.OracleProb(prob)
    ret = o.simplex(**opts)
    return ret, o.result()


_ORACLE_CACHE = {}


def _oracle_base(oracle, seed, m, n, dens, meth):
    """the oracle's plain solve of a base instance, once per session"""
    key = (seed, m, n, dens, meth)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = _oracle_run(oracle, _instance(seed, m, n, dens)[0], meth=meth)
    return _ORACLE_CACHE[key]


def _solve(ctx, prob, **opts):
    P = gk.GkProblem(ctx, prob)
    ret = gk.glp_simplex(P, gk.SMCP(msg_lev=gk.GLP_MSG_ERR, **opts))
    return P, ret


def _assert_closed_form(P, ret, prob, want, tol=None):
    """the optimum the construction promises: statuses, objective, the four
    vectors (tol: per-vector bounds, default 1e-9 each) and the certificate"""
    assert ret == 0 and (P.pbs_stat, P.dbs_stat) == (FEAS, FEAS), (ret, P.pbs_stat, P.dbs_stat)
    z = want["z"]
    err = lpgen.vector_errors(P, want)
    print(f"{prob.name}: {P.it_cnt} pivots, obj rel err {abs(P.obj_val - z) / max(1.0, abs(z)):.1e}, vectors "
          + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
    assert abs(P.obj_val - z) <= 1e-9 * max(1.0, abs(z)), (P.obj_val, z)
    for k, e in err.items():
        assert e <= (tol[k] if tol else 1e-9), (k, e, err)
    assert np.array_equal(P.row_stat[1:], want["row_stat"]) and np.array_equal(P.col_stat[1:], want["col_stat"])
    lpgen.general_kkt(P, prob)


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens,seed", SMALL)
def test_gpu_vertex_lp_matches_closed_form_and_oracle(gpu_ctx, oracle, m, n, dens, seed, meth):
    prob, want = _instance(seed, m, n, dens)
    P, ret = _solve(gpu_ctx, prob, meth=meth)
    _assert_closed_form(P, ret, prob, want)
    oret, o = _oracle_base(oracle, seed, m, n, dens, meth)
    assert (ret, P.pbs_stat, P.dbs_stat) == (oret, o["pbs_stat"], o["dbs_stat"])


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens,seed", SPARSE_A)
def test_gpu_vertex_lp_sparse_factor(gpu_ctx, oracle, monkeypatch, m, n, dens, seed, meth):
    """the sparse-A instance again on the sparse LU (GK_SPARSE=1; the run
    above takes the default factor)"""
    monkeypatch.setenv("GK_SPARSE", "1")
    prob, want = _instance(seed, m, n, dens)
    P, ret = _solve(gpu_ctx, prob, meth=meth)
    assert P.stats().factor_sparse
    _assert_closed_form(P, ret, prob, want)
    oret, o = _oracle_base(oracle, seed, m, n, dens, meth)
    assert (ret, P.pbs_stat, P.dbs_stat) == (oret, o["pbs_stat"], o["dbs_stat"])


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens,seed", PANEL)
def test_gpu_vertex_lp_default_thresholds(gpu_ctx, m, n, dens, seed, meth):
    """1030 x 2100: the MFMA panel (m >= 1024), Newton refinement (k >= 512)
    and the fone / fupd limits at their default thresholds; closed form only.
    The dual run must have been served by the panel."""
    prob, want = _instance(seed, m, n, dens)
    P, ret = _solve(gpu_ctx, prob, meth=meth)
    st = P.stats()
    print(f"panel_hits {st.panel_hits} panel_refills {st.panel_refills} refinements {st.refinements} "
          f"reinversions {st.reinversions} seconds {st.seconds_total:.2f}")
    _assert_closed_form(P, ret, prob, want)
    if meth == gk.GLP_DUAL:
        assert st.panel_hits + st.panel_refills > 0


@pytest.mark.parametrize("m,n,dens,seed", SPARSE_LU[:1])
def test_gpu_vertex_lp_default_sparse_lu(gpu_ctx, m, n, dens, seed):
    """2100 x 4300, 0.2 % dense: the default factor_choice takes the sparse LU
    (m >= 2048, 16 nnz / column <= m); closed form only.  One seed and the
    dual alone: a solve takes 16,664 pivots and 32 s on the sparse LU at this
    size (the primal 13,684 pivots and 31 s; the second seed the same), so the
    other five combinations are left out."""
    prob, want = _instance(seed, m, n, dens)
    P, ret = _solve(gpu_ctx, prob, meth=gk.GLP_DUAL)
    st = P.stats()
    print(f"factor_sparse {st.factor_sparse} reinversions {st.reinversions} seconds {st.seconds_total:.2f}")
    _assert_closed_form(P, ret, prob, want)
    assert st.factor_sparse


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("kind", ["infeasible", "unbounded"])
@pytest.mark.parametrize("m,n,dens,seed", VARIANT_SIZES)
def test_gpu_vertex_lp_infeasible_and_unbounded(gpu_ctx, oracle, m, n, dens, seed, kind, meth):
    prob = _variant(seed, m, n, dens, kind)
    P, ret = _solve(gpu_ctx, prob, meth=meth)
    oret, o = _oracle_run(oracle, prob, meth=meth)
    assert (ret, P.pbs_stat, P.dbs_stat) == (oret, o["pbs_stat"], o["dbs_stat"])
    # what the variant is built to be (both methods agree on it)
    if kind == "infeasible":
        assert P.pbs_stat == problems.GLP_NOFEAS
    else:
        assert P.dbs_stat == problems.GLP_NOFEAS


_BAD_SCALE_TOL = {}


def _bad_scale_tol(oracle, seed, scaled):
    """max(1e-9, 10 x the oracle's own error against the closed form) for each
    vector, the worse of its primal and dual solve (tests/test_lpgen.py
    test_oracle_on_bad_scale records the figures: col_prim 6e-11 .. 6e-10,
    the others <= 2e-13)"""
    key = (seed, scaled)
    if key not in _BAD_SCALE_TOL:
        m, n, dens, _ = lpgen.BAD_SCALE
        prob, want = _instance(seed, m, n, dens, True)
        p = prob.copy()
        if scaled:
            r, p.rii, p.sjj, _ = oracle.scale_prob(p.m, p.n, p.A_ptr, p.A_ind, p.A_val, gk.GLP_SF_AUTO)
            assert r == 0
        worst = dict.fromkeys(("col_prim", "row_prim", "row_dual", "col_dual"), 0.0)
        for meth in (gk.GLP_PRIMAL, gk.GLP_DUAL):
            ret, res = _oracle_run(oracle, p, meth=meth)
            assert ret == 0 and (res["pbs_stat"], res["dbs_stat"]) == (FEAS, FEAS)
            for k, e in lpgen.vector_errors(res, want).items():
                worst[k] = max(worst[k], e)
        _BAD_SCALE_TOL[key] = {k: max(1e-9, 10.0 * e) for k, e in worst.items()}
    return _BAD_SCALE_TOL[key]


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("scaled", [False, True], ids=["as-given", "sf-auto"])
@pytest.mark.parametrize("seed", lpgen.BAD_SCALE[3])
def test_gpu_vertex_lp_bad_scale(gpu_ctx, oracle, seed, scaled, meth):
    """Rows and columns scaled by 2^k, k in [-8, 8], solved as given and after
    glp_scale_prob(GLP_SF_AUTO) on the device: the scaled working set and the
    epilogue's unscaling of all four result vectors must give the closed form
    in original units."""
    m, n, dens, _ = lpgen.BAD_SCALE
    prob, want = _instance(seed, m, n, dens, True)
    P = gk.GkProblem(gpu_ctx, prob.copy())           # glp_scale_prob stores the factors in its Problem
    if scaled:
        gk.glp_set_print_func(lambda s: None)
        try:
            gk.glp_scale_prob(P, gk.GLP_SF_AUTO)
        finally:
            gk.glp_set_print_func(None)
        assert not np.all(P.rii[1:] == 1.0) and not np.all(P.sjj[1:] == 1.0)
    ret = gk.glp_simplex(P, gk.SMCP(msg_lev=gk.GLP_MSG_ERR, meth=meth))
    _assert_closed_form(P, ret, prob, want, tol=_bad_scale_tol(oracle, seed, scaled))


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens,seed", MID)
def test_gpu_vertex_lp_warm_start_takes_no_pivot(gpu_ctx, m, n, dens, seed, meth):
    """From the constructed optimal basis glp_simplex evaluates beta, pi and
    cbar at general bounds, finds nothing to do and stores the closed form:
    no pivot (the oracle does the same, tests/test_lpgen.py)."""
    prob, want = _instance(seed, m, n, dens)
    P, ret = _solve(gpu_ctx, lpgen.warm(prob, want), meth=meth)
    assert P.it_cnt == 0
    _assert_closed_form(P, ret, prob, want)


OPTIONS = [pytest.param(dict(pricing=gk.GLP_PT_STD), id="pt-std"),
           pytest.param(dict(r_test=gk.GLP_RT_STD), id="rt-std"),
           pytest.param(dict(pricing=gk.GLP_PT_STD, r_test=gk.GLP_RT_STD), id="pt-std-rt-std")]


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("opts", OPTIONS)
@pytest.mark.parametrize("m,n,dens,seed", MID)
def test_gpu_vertex_lp_non_default_options(gpu_ctx, m, n, dens, seed, opts, meth):
    """textbook pricing (the pse = 0 specialisations of the dual and primal
    kernels) and the textbook ratio test reach the same unique optimum"""
    prob, want = _instance(seed, m, n, dens)
    P, ret = _solve(gpu_ctx, prob, meth=meth, **opts)
    _assert_closed_form(P, ret, prob, want)


@pytest.mark.parametrize("meth", METHODS[1:])
@pytest.mark.parametrize("m,n,dens,seed", MID)
def test_gpu_vertex_lp_objective_limit_in_dual(gpu_ctx, oracle, m, n, dens, seed, meth):
    """obj_ll (GLP_MAX) / obj_ul (GLP_MIN) 50 away from the optimum on the
    side the dual's objective comes from: the dual stops there (GLP_EOBJLL /
    GLP_EOBJUL, dual feasible, primal infeasible) with the objective between
    the limit and the optimum, as the oracle does.  The same limit on the far
    side of the optimum changes nothing."""
    prob, want = _instance(seed, m, n, dens)
    z = want["z"]
    mx = prob.dir == problems.GLP_MAX
    name = "obj_ll" if mx else "obj_ul"
    lim = z + 50.0 if mx else z - 50.0
    P, ret = _solve(gpu_ctx, prob, meth=meth, **{name: lim})
    oret, o = _oracle_run(oracle, prob, meth=meth, **{name: lim})
    assert oret == (problems.GLP_EOBJLL if mx else problems.GLP_EOBJUL)
    assert (ret, P.pbs_stat, P.dbs_stat) == (oret, o["pbs_stat"], o["dbs_stat"])
    slack = 1e-9 * max(1.0, abs(z))
    if mx:
        assert z - slack <= P.obj_val <= lim, (P.obj_val, z, lim)
    else:
        assert lim <= P.obj_val <= z + slack, (P.obj_val, z, lim)
    far = z - 50.0 if mx else z + 50.0
    P, ret = _solve(gpu_ctx, prob, meth=meth, **{name: far})
    _assert_closed_form(P, ret, prob, want)


@pytest.mark.parametrize("meth", [METHODS[0], METHODS[2]])
@pytest.mark.parametrize("m,n,dens,seed", STOPPED)
def test_gpu_vertex_lp_it_lim_state_matches_oracle(gpu_ctx, oracle, m, n, dens, seed, meth):
    """Stopped after 150 pivots, with phase I still running for general
    bounds: GLP_EITLIM, exactly 150 pivots, and the oracle's state after the
    same call: every row and column status and the objective."""
    prob, _ = _instance(seed, m, n, dens)
    P, ret = _solve(gpu_ctx, prob, meth=meth, it_lim=150)
    oret, o = _oracle_run(oracle, prob, meth=meth, it_lim=150)
    assert ret == oret == problems.GLP_EITLIM and P.it_cnt == o["it_cnt"] == 150
    assert (P.pbs_stat, P.dbs_stat) == (o["pbs_stat"], o["dbs_stat"])
    rs = np.asarray(P.row_stat[1:]) != o["row_stat"]
    cs = np.asarray(P.col_stat[1:]) != o["col_stat"]
    assert not rs.any() and not cs.any(), (f"{int(rs.sum())} row / {int(cs.sum())} column statuses differ; first "
                                           f"rows {np.nonzero(rs)[0][:5] + 1}, cols {np.nonzero(cs)[0][:5] + 1}")
    assert abs(P.obj_val - o["obj_val"]) <= 1e-9 * max(1.0, abs(o["obj_val"])), (P.obj_val, o["obj_val"])
