"""Implicit-feedback ALS (cf_ials.hip, CFImplicitALSEngine) on the GPU: the
side Gram exactly, every solved row against its own f64 normal equations on
the two-sided degree ladder (fused rows and hub chunks on both sides), two
partitions, the objective, and the public interface."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import degree_ladder as dl  # noqa: E402
from test_gpu_cf import _rand_init, _sync_parts  # noqa: E402

from lux_amd import cpu_ref  # noqa: E402
from lux_amd.cf_engine import als_init  # noqa: E402
from lux_amd.cf_ials_engine import CFImplicitALSEngine  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, REG = 40.0, 0.01
F32_TOL, HUB_TOL = 5e-5, 2e-4  # the project's residual tolerances


@functools.lru_cache(maxsize=None)
def _lad():
    return dl.bipartite_ladder(nu=128, ni=131)  # 131: tail of 3 mod 4 and 32


def _ladder_part():
    full = DeviceCSC.from_host(_lad().g)
    full.n_users = _lad().nu
    return GraphPart(full, 1, 0)


def _engine(part, K, init):
    eng = CFImplicitALSEngine(part, K=K, alpha=ALPHA, reg=REG)
    eng.old.copy_(torch.from_numpy(np.ascontiguousarray(init).ravel()))
    return eng


def _vec(eng):
    return eng.vectors().cpu().numpy().copy()


def _check_phase(g, nu, basis, after, side, K):
    """Every row of `side` satisfies ITS OWN A_v x = b_v, assembled in f64
    from `basis` (what the phase read), in _phase_residual's metric; rows
    without entries are zero and the other side keeps its bits."""
    lo, hi = (0, nu) if side == "users" else (nu, g.nv)
    Y = (basis[nu:] if side == "users" else basis[:nu]).astype(np.float64)
    base = Y.T @ Y + REG * np.eye(K)
    b = 0 if lo == 0 else int(g.col_end[lo - 1])
    worst = 0.0
    for v in range(lo, hi):
        e = int(g.col_end[v])
        if e == b:
            assert not after[v].any(), f"zero-entry row {v}"
            continue
        S = basis[g.src[b:e]].astype(np.float64)
        w = g.weight[b:e].astype(np.float64)
        A = base + ALPHA * (S.T * w) @ S
        rhs = (1.0 + ALPHA * w) @ S
        x = after[v].astype(np.float64)
        rel = np.linalg.norm(A @ x - rhs) / (
            np.linalg.norm(A, ord=np.inf) * np.linalg.norm(x)
            + np.linalg.norm(rhs))
        worst = max(worst, rel)
        tol = HUB_TOL if e - b >= dl.T2 else F32_TOL
        assert rel < tol, f"row {v} degree {e - b}: residual {rel:.3g}"
        b = e
    print(f"{side} K={K}: worst residual {worst:.3g}")
    other = np.ones(g.nv, bool)
    other[lo:hi] = False
    assert np.array_equal(after[other].view(np.uint32),
                          basis[other].view(np.uint32))


def _check_gram(eng, F, nu, K):
    for side, sl in (("users", slice(0, nu)), ("items", slice(nu, None))):
        got = eng.side_gram(side).cpu().numpy()
        Y = F[sl].astype(np.int64)
        want = np.zeros((64, 64), np.int64)
        want[:K, :K] = Y.T @ Y
        assert np.array_equal(got, want), side  # no tolerance
        assert np.array_equal(got, got.T) and not got[K:].any() \
            and not got[:, K:].any()
        again = eng.side_gram(side).cpu().numpy()
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("K", [1, 20, 64])
def test_side_gram_exact(K):
    """Integer factors 0..6 (36 * 131 < 2^24: fp32 is exact in any order):
    both sides' Gram EQUALS the int64 Y^T Y. 128 rows = 4 full one-tile
    slabs; 131 = a fifth slab of 3 rows."""
    lad = _lad()
    F = dl.int_factors(lad.g.nv, K)
    _check_gram(_engine(_ladder_part(), K, F), F, lad.nu, K)


@pytest.mark.parametrize("K", [20, 64])
def test_side_gram_multi_tile_slabs(K):
    """70001 user rows: 1024 workgroups are not enough for one tile each, so
    every slab is 96 rows = 3 tiles through the register prefetch, the last
    slab ragged (36 * 70001 < 2^24: still exact)."""
    nu, ni = 70001, 96
    full = DeviceCSC.bipartite(nu, ni, 20000, seed=5)
    F = dl.int_factors(nu + ni, K)
    _check_gram(_engine(GraphPart(full, 1, 0), K, F), F, nu, K)


@pytest.mark.parametrize("K", [20, 64])
def test_residual_ladder(K):
    """alpha = 40, reg = 0.01 from a random init, over every degree at which
    a kernel, a tile loop or a chunk loop changes path, hubs on both sides.
    An fp32 numpy emulation of the algorithm on this input (sqrt scaling
    included) measured worst 4.0e-7 and smallest pivot/diagonal 8.5e-3: the
    tolerances sit > 100x above fp32 and the 1e-5 pivot floor marks nothing."""
    lad = _lad()
    nu = lad.nu
    init = _rand_init(lad.g.nv, K, seed=42)
    eng = _engine(_ladder_part(), K, init)
    assert eng.nbigu == len(dl.LADDER_CHUNK) == eng.part.nbig - eng.nbigu
    eng.half_step("users")
    got_u = _vec(eng)
    _check_phase(lad.g, nu, init, got_u, "users", K)
    eng.half_step("items")
    got_i = _vec(eng)
    _check_phase(lad.g, nu, got_u, got_i, "items", K)
    twin = _engine(_ladder_part(), K, init)  # its own bin build and lists
    twin.step()
    assert np.array_equal(_vec(twin).view(np.uint32), got_i.view(np.uint32))


def test_two_partitions():
    """Phase-locked partitions, _sync_parts standing in for the all-gather:
    each computes the whole opposite-side Gram itself."""
    nu, ni, ne, K = 1000, 256, 40000, 32
    full = DeviceCSC.bipartite(nu, ni, ne, seed=19)
    g = Graph.bipartite(nu, ni, ne, seed=19)
    init = _rand_init(nu + ni, K, seed=77)
    ea = _engine(GraphPart(full, 2, 0, keep_full=True), K, init)
    eb = _engine(GraphPart(full, 2, 1), K, init)
    for _ in range(2):
        for side in ("users", "items"):
            basis = _vec(ea)
            ea.half_step(side)
            eb.half_step(side)
            _sync_parts((ea, eb), K)
            _check_phase(g, nu, basis, _vec(ea), side, K)
    assert np.array_equal(_vec(ea).view(np.uint32), _vec(eb).view(np.uint32))


def test_objective_decreases():
    """Each phase minimises cf_ials_loss exactly and three sweeps from
    als_init are far from convergence: strictly smaller after every sweep."""
    nu, ni, ne, K = 300, 200, 6000, 32
    g = Graph.bipartite(nu, ni, ne, seed=9)
    eng = CFImplicitALSEngine(
        GraphPart(DeviceCSC.bipartite(nu, ni, ne, seed=9), 1, 0), K=K,
        alpha=ALPHA, reg=REG)
    assert np.array_equal(_vec(eng), als_init(nu + ni, K).reshape(-1, K))
    loss = [cpu_ref.cf_ials_loss(g, K, _vec(eng), ALPHA, REG, nu)]
    for _ in range(3):
        eng.step()
        loss.append(cpu_ref.cf_ials_loss(g, K, _vec(eng), ALPHA, REG, nu))
        print(loss[-2:])
        assert loss[-1] < loss[-2]


def test_interface():
    part = _ladder_part()
    with pytest.raises(ValueError, match="64"):
        CFImplicitALSEngine(part, K=65)
    part.n_users = None
    with pytest.raises(ValueError, match="-users"):
        CFImplicitALSEngine(part, K=20)
    part = _ladder_part()
    part.weight = part.weight.clone()
    part.weight[5] = -1
    with pytest.raises(ValueError, match="weight"):
        CFImplicitALSEngine(part, K=20)
    r = subprocess.run(
        [sys.executable, "-m", "lux_amd.apps.cf", "-synthetic",
         "bipartite:300:200:6000", "-als", "-implicit", "-k", "32", "-ni", "2",
         "-topn", "5", "-queries", "4"],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "check() = 0" in r.stdout and "alpha = 40" in r.stdout
    r = subprocess.run(
        [os.path.join(ROOT, "bin", "col_filter"), "-synthetic",
         "bipartite:300:200:6000", "-als", "-implicit"],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "lux_amd.apps.cf" in r.stderr
