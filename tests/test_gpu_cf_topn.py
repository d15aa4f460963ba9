"""CF top-N (CFTopN, src/gpu/cf_topn.hip) against the numpy oracle
cpu_ref.cf_topn: integer factors held to equality over the edge values of
every axis, bit-identity across work splits and runs, trained factors held to
the fp32 rounding bound of a K-term dot product against f64, validation and
the app."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lux_amd import cpu_ref  # noqa: E402
from lux_amd.cf_engine import CFALSEngine  # noqa: E402
from lux_amd.cf_topn_engine import CFTopN  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = (64, 129, 65, 10)  # K, candidates, queries, n
LADDER = [BASE, (1, 1, 1, 1), (128, 193, 65, 64)] + \
    [(K, 129, 65, 10) for K in (1, 3, 4, 20, 32, 33, 65, 128)] + \
    [(64, C, 65, 10) for C in (1, 15, 16, 17, 63, 64, 65, 193)] + \
    [(64, 129, Q, 10) for Q in (1, 15, 16, 17, 64)] + \
    [(64, 129, 65, n) for n in (1, 64)]


def _stub(nv, nparts=1):
    """What topn() needs of a GraphPart: the vertex count and the device."""
    return types.SimpleNamespace(
        nv=nv, nparts=nparts, n_users=None,
        col=torch.zeros(1, dtype=torch.int32, device="cuda:0"))


def _case(K, C, Q, n, real=False):
    """Queries 0..Q-1 (the last repeats the first), candidates [Q, Q + C),
    and per query vertex p an exclusion row by p % 4: empty, one entry, every
    candidate, all but n - 1."""
    rng = np.random.default_rng(1000 * K + 10 * C + Q + n)
    vec = rng.standard_normal((Q + C, K)).astype(np.float32) if real else \
        rng.integers(-4, 5, (Q + C, K)).astype(np.float32)
    queries = np.arange(Q)
    queries[-1] = 0
    cand = np.arange(Q, Q + C)
    rows = [[np.empty(0, np.int64), rng.choice(cand, 1), cand,
             np.sort(rng.choice(cand, max(C - (n - 1), 0), replace=False))
             ][p % 4] for p in range(Q)] + [np.empty(0, np.int64)] * C
    ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    adj = np.concatenate(rows + [np.zeros(1, np.int64)])  # never empty
    return vec, queries, ptr, adj


def _run(K, C, Q, n, real=False):
    vec, queries, ptr, adj = _case(K, C, Q, n, real)
    rec = CFTopN(_stub(Q + C), torch.from_numpy(vec).cuda())
    items, scores = rec.topn(
        queries, Q, Q + C, n, torch.from_numpy(ptr).cuda(),
        torch.from_numpy(adj.astype(np.int32)).cuda())
    return rec, items.cpu(), scores.cpu()


# ---- 1. exact ladder ----

@pytest.mark.parametrize("K,C,Q,n", LADDER)
def test_integer_factors_equal_the_oracle(K, C, Q, n):
    vec, queries, ptr, adj = _case(K, C, Q, n)
    want_i, want_s = cpu_ref.cf_topn(vec, queries, Q, Q + C, n, ptr, adj)
    rec, items, scores = _run(K, C, Q, n)
    assert torch.equal(items, torch.from_numpy(want_i))
    assert torch.equal(scores, torch.from_numpy(want_s.astype(np.float32)))
    assert rec.check() == 0


# ---- 2. split invariance ----

@pytest.mark.parametrize("case", [BASE, (64, 193, 65, 10)])
def test_every_split_gives_the_same_bits(case, monkeypatch):
    monkeypatch.delenv("LUX_CF_TOPN_SPLIT", raising=False)
    rec, items, scores = _run(*case, real=True)
    assert rec.stats["splits"] > 1 and rec.stats["launches"] == 2
    for split in ("1", "2", "3", "4", "1"):
        monkeypatch.setenv("LUX_CF_TOPN_SPLIT", split)
        rec, it, sc = _run(*case, real=True)
        assert (rec.stats["splits"] == 1) == (split == "1")
        assert rec.stats["splits"] <= int(split)
        assert torch.equal(it, items)
        assert torch.equal(sc.view(torch.int32), scores.view(torch.int32))


# ---- 3. trained factors against f64 ----

@functools.lru_cache(maxsize=None)
def _trained(K):
    part = GraphPart(DeviceCSC.bipartite(300, 200, 6000, device="cuda:0"),
                     1, 0)
    eng = CFALSEngine(part, K=K)
    eng.step()
    eng.step()
    ptr = part.row_ptr.cpu().numpy()
    col = part.col.cpu().numpy()
    seen = np.zeros((part.nv, part.nv), bool)
    seen[np.repeat(np.arange(part.nv), np.diff(ptr)), col] = True
    return part, eng.vectors().clone(), seen


def _within_bound(vec, queries, cand, admissible, items, scores):
    """The four per-row properties, tol = 2 K 2^-24 sum |u_k v_k| in f64."""
    v = vec.double().cpu().numpy()
    K, rows = v.shape[1], np.arange(queries.size)[:, None]
    ref = v[queries] @ v[cand].T
    tol = 2 * K * 2.0 ** -24 * (np.abs(v[queries]) @ np.abs(v[cand]).T)
    items, scores = items.numpy(), scores.numpy().astype(np.float64)
    assert (items >= cand[0]).all() and (items <= cand[-1]).all()
    at = items - cand[0]
    assert admissible[rows, at].all()
    assert (np.diff(np.sort(items, axis=1), axis=1) > 0).all()
    assert (np.abs(scores - ref[rows, at]) <= tol[rows, at]).all()
    s0, s1, i0, i1 = scores[:, :-1], scores[:, 1:], items[:, :-1], items[:, 1:]
    assert ((s0 > s1) | ((s0 == s1) & (i0 < i1))).all()
    out = admissible.copy()
    out[rows, at] = False
    last = at[:, -1:]
    bound = ref[rows, last] + tol[rows, last] + tol
    assert (ref <= bound)[out].all()


@pytest.mark.parametrize("K", [20, 64])
def test_trained_factors_within_the_rounding_bound(K):
    part, vec, seen = _trained(K)
    nu, nv = part.n_users, part.nv
    rec = CFTopN(part, vec)
    cand = np.arange(nu, nv)
    users = np.arange(nu)
    items, scores = rec.recommend(users, n=10)
    assert rec.check() == 0
    items, scores = items.cpu(), scores.cpu()
    _within_bound(vec, users, cand, ~seen[:nu, nu:], items, scores)
    wrong = items.clone()
    wrong[7, 0] = wrong[7, 1]
    assert rec.check(wrong, scores) > 0
    items, scores = rec.similar(cand, n=10)
    assert rec.check() == 0
    _within_bound(vec, cand, cand, ~np.eye(nv - nu, dtype=bool), items.cpu(),
                  scores.cpu())


# ---- 4. validation and the app ----

def test_arguments_are_validated():
    part, vec, _ = _trained(20)
    nu, nv = part.n_users, part.nv
    with pytest.raises(ValueError, match="single-rank"):
        CFTopN(_stub(nv, nparts=2), vec)
    for bad in (vec.double(), vec[:-1], vec.cpu(), vec.view(-1),
                torch.zeros((nv, 129), device="cuda:0")):
        with pytest.raises(ValueError):
            CFTopN(part, bad)
    rec = CFTopN(part, vec)
    with pytest.raises(ValueError, match="no result yet"):
        rec.check()
    for users in ([nu], [-1], [], [0.5], torch.tensor([[0]])):
        with pytest.raises(ValueError):
            rec.recommend(users)
    with pytest.raises(ValueError):
        rec.similar([0])
    for n in (0, 65, 2.0):
        with pytest.raises(ValueError, match="n must be"):
            rec.recommend([0], n=n)
    for c_lo, c_hi in ((5, 5), (0, nv + 1), (-1, 4)):
        with pytest.raises(ValueError, match="candidates"):
            rec.topn([0], c_lo, c_hi, 3)
    ptr = torch.zeros(nv + 1, dtype=torch.int64, device="cuda:0")
    adj = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    for p, a in ((ptr, None), (ptr[:-1], adj), (ptr.int(), adj),
                 (ptr, adj.long()), (ptr.cpu(), adj)):
        with pytest.raises(ValueError):
            rec.topn([0], nu, nv, 3, p, a)
    with pytest.raises(RuntimeError, match="n_users is unset"):
        CFTopN(_stub(nv), vec).recommend([0])


@pytest.mark.parametrize("topn", [["-topn", "5", "-queries", "70"], []])
def test_app_in_a_child_process(topn):
    r = subprocess.run(
        [sys.executable, "-m", "lux_amd.apps.cf", "-synthetic",
         "bipartite:300:200:6000", "-als", "-k", "20", "-ni", "2"] + topn,
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ELAPSED TIME" in r.stdout
    if topn:
        assert "TOPN TIME" in r.stdout and "check() = 0" in r.stdout
        assert r.stdout.count("\nuser ") == 3
    else:
        assert "TOPN" not in r.stdout and "check()" not in r.stdout
