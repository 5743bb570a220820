"""The dual batch plan's cap of the dense-column list (ST_CAP).

A batch is planned for a list of up to nr_cap = bucket(nr + GK_PLAN_SLACK)
dense columns of inv(B); a pivot that could take the list past the cap stops
the batch with ST_CAP before it stores anything, and the host plans the next
batch from the new length.  The cap only cuts the pivots into batches: the
pivot path, the pivot count and what the call returns do not depend on it.

All on gen_dense(256, 1024, seed=42), the smallest dense shape that takes the
row path with the fused update and whose list crosses several 64-wide
buckets on its way from the slack basis to the optimum (1,252 pivots).  The
reference is the oracle's full dual solve of the same instance, computed once
for the module; the objective is compared as tests/test_gpu_lp.py compares
the dense fixtures (1e-9 relative), the pivot count for equality.
"""
import numpy as np
import pytest

from glpk_js_amd import gk, problems

pytestmark = pytest.mark.gpu

SLACKS = {"slack1": "1", "default": None, "today": "1000"}      # (>= any batch size: the sizing before the cap)


@pytest.fixture(scope="module")
def prob():
    return problems.gen_dense(256, 1024, seed=42)


@pytest.fixture(scope="module")
def ref(oracle, prob):
    o = oracle.OracleProb(prob)
    ret = o.simplex(meth=3)
    r = o.result()
    return {"ret": ret, "it_cnt": int(r["it_cnt"]), "obj_val": float(r["obj_val"]),
            "pbs_stat": r["pbs_stat"], "dbs_stat": r["dbs_stat"]}


def _setenv(monkeypatch, slack):
    if slack is None:
        monkeypatch.delenv("GK_PLAN_SLACK", raising=False)
    else:
        monkeypatch.setenv("GK_PLAN_SLACK", slack)


def _solve(ctx, prob, **opts):
    P = gk.GkProblem(ctx, prob)
    ret = gk.glp_simplex(P, gk.SMCP(meth=gk.GLP_DUAL, msg_lev=gk.GLP_MSG_ERR, **opts))
    return P, ret


def test_gpu_full_dual_solve_under_three_caps(gpu_ctx, prob, ref, monkeypatch):
    """Slack 1, the default and a slack of at least the batch size: each run
    returns 0 with the oracle's pivot count, statuses and objective, and the
    slack-1 run needs more batches than the default (the ST_CAP path ran)."""
    assert ref["ret"] == 0
    batches = {}
    for name, slack in SLACKS.items():
        _setenv(monkeypatch, slack)
        P, ret = _solve(gpu_ctx, prob)
        batches[name] = int(P.stats().batches)
        rel = abs(P.obj_val - ref["obj_val"]) / max(1.0, abs(ref["obj_val"]))
        print(f"{name}: ret {ret}, {P.it_cnt} pivots (oracle {ref['it_cnt']}), obj {P.obj_val!r} "
              f"(oracle {ref['obj_val']!r}, rel {rel:.1e}), {batches[name]} batches")
        assert ret == 0
        assert (P.pbs_stat, P.dbs_stat) == (ref["pbs_stat"], ref["dbs_stat"])
        assert P.it_cnt == ref["it_cnt"]
        assert rel <= 1e-9, (P.obj_val, ref["obj_val"])
    assert batches["slack1"] > batches["default"], batches


CHAIN_CALLS = 100       # 700 pivots: the list grows from 0 to ≈155 entries, across the buckets at 64 and 128


def _chain(ctx, prob):
    P = gk.GkProblem(ctx, prob)
    parm = gk.SMCP(meth=gk.GLP_DUAL, msg_lev=gk.GLP_MSG_ERR, it_lim=7)
    out, batches = [], 0
    for _ in range(CHAIN_CALLS):
        ret = gk.glp_simplex(P, parm)
        batches += int(P.stats().batches)
        out.append((ret, P.it_cnt, P.obj_val, np.asarray(P.row_stat[1:], np.int8).tobytes(),
                    np.asarray(P.col_stat[1:], np.int8).tobytes()))
    return out, batches


def test_gpu_it_lim_chain_with_cap_stops(gpu_ctx, oracle, prob, monkeypatch):
    """Calls of it_lim=7 with slack 1: every call's one batch ends in the
    end-of-call epilogue, and the calls in which the list crosses a bucket
    stop on the cap first and finish in one batch more.  After every call the
    return code, the pivot count, the statuses and the objective (1e-9
    relative) are those of the oracle carried along the same calls, and the
    chain planned with the sizing before the cap gives the same.

    (The reference restarts phase I in every call, so a chain of short calls
    does not follow the pivots of one long call: the oracle's own it_lim=7
    chain of this instance is at objective 229.37 after 1,200 calls and 8,400
    pivots, and its it_lim=100 chain needs 2,864 pivots, where one call
    reaches 240.269 after 1,252.  The chain is therefore held against the
    oracle's chain, call by call, not against the long call.)"""
    o = oracle.OracleProb(prob)
    want = []
    for _ in range(CHAIN_CALLS):
        oret = o.simplex(meth=3, it_lim=7)
        r = o.result()
        want.append((oret, int(r["it_cnt"]), float(r["obj_val"]), np.asarray(r["row_stat"], np.int8).tobytes(),
                     np.asarray(r["col_stat"], np.int8).tobytes()))
    _setenv(monkeypatch, "1")
    got, batches = _chain(gpu_ctx, prob)
    _setenv(monkeypatch, SLACKS["today"])
    base, batches_base = _chain(gpu_ctx, prob)
    worst = max(abs(g[2] - w[2]) / max(1.0, abs(w[2])) for g, w in zip(got, want))
    print(f"chain of {CHAIN_CALLS} calls: {got[-1][1]} pivots (oracle {want[-1][1]}), obj {got[-1][2]!r} "
          f"(oracle {want[-1][2]!r}), worst rel {worst:.1e}; batches {batches} with slack 1, {batches_base} before")
    for k, (g, w, b) in enumerate(zip(got, want, base)):
        assert g[:2] == w[:2] == b[:2] == (problems.GLP_EITLIM, 7 * (k + 1)), (k, g[:2], w[:2], b[:2])
        assert g[3:] == w[3:] == b[3:], k
        assert abs(g[2] - w[2]) <= 1e-9 * max(1.0, abs(w[2])), (k, g[2], w[2])
        assert abs(b[2] - w[2]) <= 1e-9 * max(1.0, abs(w[2])), (k, b[2], w[2])
    assert batches > batches_base >= CHAIN_CALLS, (batches, batches_base)


def test_gpu_cap_stops_repeatable(gpu_ctx, prob, monkeypatch):
    """Two solves with slack 1 return the same arrays, bit for bit."""
    _setenv(monkeypatch, "1")
    runs = []
    for _ in range(2):
        P, ret = _solve(gpu_ctx, prob)
        r = P.result()
        runs.append((ret, int(P.stats().batches),
                     {k: np.asarray(v).tobytes() for k, v in r.items()}))
    assert runs[0][0] == 0
    assert runs[1] == runs[0]
