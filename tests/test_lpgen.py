"""The closed-form LP generator (tests/lpgen.py) against the oracle, on the
CPU: every instance the GPU tests use with m <= lpgen.ORACLE_MAX_M is solved
by the oracle alone, with both methods, to the vectors the construction
promises.  This is the generator's admission test: an instance that fails here
gets another seed, never a wider bound.  general_kkt is checked both ways: it
accepts the oracle's optimum and every recorded optimum of the lp_* fixtures,
and rejects a stopped run, a flipped dual and a column off its bound."""
import functools
import os

import numpy as np
import pytest

import lpgen
import orcpy
from conftest import golden_files, load_golden
from glpk_js_amd import gk, problems

FEAS = problems.GLP_FEAS
SMALL = [pytest.param(m, n, dens, seed, id=f"{m}x{n}-d{dens}-s{seed}")
         for (m, n, dens, seeds) in lpgen.INSTANCES if m <= lpgen.ORACLE_MAX_M for seed in seeds]
METHODS = [pytest.param(gk.GLP_PRIMAL, id="primal"), pytest.param(gk.GLP_DUAL, id="dual")]


@functools.lru_cache(maxsize=None)
def _instance(seed, m, n, dens, bad_scale=False):
    return lpgen.gen_vertex(seed, m, n, dens, bad_scale)


@functools.lru_cache(maxsize=None)
def _solved(seed, m, n, dens, meth):
    prob, _ = _instance(seed, m, n, dens)
    o = orcpy.OracleProb(prob)
    ret = o.simplex(meth=meth)
    return ret, o.result()


def test_each_size_has_both_directions():
    for (m, n, dens, seeds) in lpgen.INSTANCES + (lpgen.BAD_SCALE,):
        dirs = {lpgen.gen_vertex(s, m, n, dens)[0].dir for s in seeds}
        assert dirs == {problems.GLP_MIN, problems.GLP_MAX}, (m, n, dirs)


@pytest.mark.parametrize("m,n,dens,seed", SMALL)
def test_construction_is_a_nondegenerate_vertex(m, n, dens, seed):
    """exactly m basic variables, each at least 1 inside its bounds with zero
    dual; the others on a bound with a dual of 0.5 .. 5; c = A'y + d; the
    closed form passes the certificate"""
    prob, want = _instance(seed, m, n, dens)
    stat = np.concatenate([want["row_stat"], want["col_stat"]])
    typ = np.concatenate([prob.row_type, prob.col_type])
    v = np.concatenate([want["r"], want["x"]])
    dual = np.concatenate([want["y"], want["d"]])
    lb = np.concatenate([prob.row_lb, prob.col_lb])
    ub = np.concatenate([prob.row_ub, prob.col_ub])
    b = stat == problems.GLP_BS
    assert int(b.sum()) == m
    assert b[typ == problems.GLP_FR].all() and not b[typ == problems.GLP_FX].any()
    lo = b & np.isin(typ, (problems.GLP_LO, problems.GLP_DB))
    up = b & np.isin(typ, (problems.GLP_UP, problems.GLP_DB))
    assert (v[lo] - lb[lo]).min(initial=9.0) >= 1.0 and (ub[up] - v[up]).min(initial=9.0) >= 1.0
    assert np.all(dual[b] == 0.0)
    assert np.abs(dual[~b]).min() >= 0.5 and np.abs(dual[~b]).max() <= 5.0
    assert np.count_nonzero(prob.dense, axis=0).min() >= 1 and prob.c0 != 0.0
    assert np.array_equal(prob.dense @ want["x"], want["r"])
    sol = dict(obj_val=want["z"], row_stat=want["row_stat"], col_stat=want["col_stat"], row_prim=want["r"],
               col_prim=want["x"], row_dual=want["y"], col_dual=want["d"])
    lpgen.general_kkt(sol, prob, tol=1e-12)


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens,seed", SMALL)
def test_oracle_reproduces_closed_form(m, n, dens, seed, meth):
    prob, want = _instance(seed, m, n, dens)
    ret, r = _solved(seed, m, n, dens, meth)
    assert ret == 0 and (r["pbs_stat"], r["dbs_stat"]) == (FEAS, FEAS)
    assert abs(r["obj_val"] - want["z"]) <= 1e-12 * max(1.0, abs(want["z"])), (r["obj_val"], want["z"])
    err = lpgen.vector_errors(r, want)
    assert max(err.values()) <= 1e-9, err
    assert np.array_equal(r["row_stat"], want["row_stat"]) and np.array_equal(r["col_stat"], want["col_stat"])
    lpgen.general_kkt(r, prob)


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens,seed", SMALL)
def test_general_kkt_rejects_wrong_answers(m, n, dens, seed, meth):
    prob, want = _instance(seed, m, n, dens)
    _, r = _solved(seed, m, n, dens, meth)
    # a run stopped early is not optimal
    o = orcpy.OracleProb(prob)
    assert o.simplex(meth=meth, it_lim=50) == problems.GLP_EITLIM
    with pytest.raises(AssertionError):
        lpgen.general_kkt(o.result(), prob)
    # one dual with the wrong sign: a non-basic row's and a non-basic column's
    for key, stat in (("row_dual", "row_stat"), ("col_dual", "col_stat")):
        bad = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in r.items()}
        k = int(np.nonzero((bad[stat] == problems.GLP_NL) | (bad[stat] == problems.GLP_NU))[0][0])
        bad[key][k] = -bad[key][k]
        with pytest.raises(AssertionError):
            lpgen.general_kkt(bad, prob)
    # one non-basic column moved off its bound
    bad = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in r.items()}
    k = int(np.nonzero(bad["col_stat"] != problems.GLP_BS)[0][0])
    bad["col_prim"][k] += 0.25
    with pytest.raises(AssertionError):
        lpgen.general_kkt(bad, prob)


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens,seed", [p for p in SMALL if p.values[0] in (130, 270)])
def test_oracle_warm_start_from_known_basis_takes_no_pivot(m, n, dens, seed, meth):
    prob, want = _instance(seed, m, n, dens)
    o = orcpy.OracleProb(lpgen.warm(prob, want))
    assert o.simplex(meth=meth) == 0
    r = o.result()
    assert (r["pbs_stat"], r["dbs_stat"], r["it_cnt"]) == (FEAS, FEAS, 0)
    assert max(lpgen.vector_errors(r, want).values()) <= 1e-9
    lpgen.general_kkt(r, prob)


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("m,n,dens", [(130, 300, 0.6), (300, 700, 0.4)])
def test_oracle_on_infeasible_and_unbounded_variants(m, n, dens, meth):
    seeds = next(s for (mm, nn, _, s) in lpgen.INSTANCES if (mm, nn) == (m, n))
    for seed in seeds:
        prob, want = _instance(seed, m, n, dens)
        o = orcpy.OracleProb(lpgen.infeasible(prob, want))
        assert o.simplex(meth=meth) == 0 and o.result()["pbs_stat"] == problems.GLP_NOFEAS
        o = orcpy.OracleProb(lpgen.unbounded(prob))
        assert o.simplex(meth=meth) == 0 and o.result()["dbs_stat"] == problems.GLP_NOFEAS


def bad_scale_oracle_errors(seed, scaled):
    """The oracle's own error on a bad_scale instance: for each vector the
    larger of the primal and the dual solve's error against the closed form,
    as given (scaled False) or with GLP_SF_AUTO factors (scaled True)."""
    m, n, dens, _ = lpgen.BAD_SCALE
    prob, want = _instance(seed, m, n, dens, True)
    p = prob.copy()
    if scaled:
        ret, p.rii, p.sjj, _ = orcpy.scale_prob(p.m, p.n, p.A_ptr, p.A_ind, p.A_val, gk.GLP_SF_AUTO)
        assert ret == 0
    worst = {}
    for meth in (gk.GLP_PRIMAL, gk.GLP_DUAL):
        o = orcpy.OracleProb(p)
        assert o.simplex(meth=meth) == 0
        r = o.result()
        assert (r["pbs_stat"], r["dbs_stat"]) == (FEAS, FEAS)
        assert abs(r["obj_val"] - want["z"]) <= 1e-12 * max(1.0, abs(want["z"]))
        lpgen.general_kkt(r, prob)
        for k, e in lpgen.vector_errors(r, want).items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


@pytest.mark.parametrize("scaled", [False, True], ids=["as-given", "sf-auto"])
@pytest.mark.parametrize("seed", lpgen.BAD_SCALE[3])
def test_oracle_on_bad_scale(seed, scaled, capsys):
    """Rows and columns scaled by 2^k, k in [-8, 8], 270 x 530.  The oracle
    reaches the optimum (objective to 1e-12, certificate accepted); its vector
    errors against the closed form are recorded, not bounded in advance: the
    GPU test takes max(1e-9, 10 x these) as its tolerance.  Measured (worst of
    primal and dual, relative to 1 + max-abs of the vector):

      seed 1 as given: col_prim 2.3e-10, row_prim 1.2e-14, row_dual 4.5e-15, col_dual 8.6e-14
      seed 1 SF_AUTO:  col_prim 6.0e-10, row_prim 2.2e-14, row_dual 5.1e-15, col_dual 6.7e-14
      seed 2 as given: col_prim 6.3e-11, row_prim 1.5e-15, row_dual 8.1e-15, col_dual 1.6e-13
      seed 2 SF_AUTO:  col_prim 1.8e-10, row_prim 5.7e-15, row_dual 1.0e-14, col_dual 2.1e-13"""
    err = bad_scale_oracle_errors(seed, scaled)
    with capsys.disabled():
        print(f"\nbad_scale seed {seed} {'SF_AUTO' if scaled else 'as given'}: oracle errors "
              + ", ".join(f"{k} {v:.1e}" for k, v in err.items()))
    assert all(np.isfinite(v) for v in err.values())
    if scaled:
        p = _instance(seed, *lpgen.BAD_SCALE[:3], True)[0]
        _, rii, sjj, _ = orcpy.scale_prob(p.m, p.n, p.A_ptr, p.A_ind, p.A_val, gk.GLP_SF_AUTO)
        assert not np.all(rii == 1.0) and not np.all(sjj == 1.0)


FIXTURE_OPTIMA = []
for _path in golden_files("lp_"):
    for _r, _run in enumerate(load_golden(_path)["runs"]):
        if not _run["opts"].get("it_lim") and _run.get("pbs_stat") == FEAS and _run.get("dbs_stat") == FEAS:
            FIXTURE_OPTIMA.append(pytest.param(_path, _r, id=f"{os.path.basename(_path)[3:-5]}-{_r}"))


@pytest.mark.parametrize("path,run_index", FIXTURE_OPTIMA)
def test_general_kkt_accepts_recorded_fixture_optima(path, run_index):
    """every optimum the reference recorded in tests/golden/lp_*.json passes
    the certificate test_gpu_lp.py applies to the GPU's answer"""
    d = load_golden(path)
    run = d["runs"][run_index]
    lpgen.general_kkt(run, problems.from_fixture(d))
