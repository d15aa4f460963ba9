"""ALS at latent rank 64 < K <= 128 (cf_als.hip wide path): the 8x8 MFMA
tile grid split over two waves, the packed 128-row Cholesky, the 128-pitch
hub scratch, through CFALSEngine and bin/col_filter.

Which case reaches which kernel (ladder degree, Gram mode):
  cf_als_wide_solve_kernel<0|1>       degrees 1..2047
  cf_als_wide_gram_chunk_kernel<0|1>  degrees >= 2048, 8192-edge chunks
  cf_als_wide_hub_solve_kernel        degrees >= 2048

The ladder is bipartite_ladder(384, 384), not the default 128/128: at
K = 128 a hub row over only 128 distinct sources is numerically rank
deficient, the pivot rule then (correctly) takes no step along some
directions and the residual contract does not apply. With 384 sources per
side an fp32 emulation of the kernel's Cholesky marks no deficient pivot,
and every ladder degree is still present on both sides.

Tolerances are the project's own (5e-5 fused rows, 2e-4 hub rows, 5e-2
bf16) in _phase_residual's metric; an fp32 CPU reference of the same
algorithm stays below 4e-7 on this input, so they stand > 100x above what
fp32 alone produces.
"""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import degree_ladder as dl  # noqa: E402
from test_gpu_cf import _phase_residual, _rand_init, _sync_parts  # noqa: E402

from lux_amd import checkpoint as ck  # noqa: E402
from lux_amd import cpu_ref  # noqa: E402
from lux_amd.cf_engine import CFALSEngine, CFEngine, als_init  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
KP = 128
F32_TOL, HUB_TOL, BF16_TOL = 5e-5, 2e-4, 5e-2  # the project's tolerances


@functools.lru_cache(maxsize=None)
def _lad():
    return dl.bipartite_ladder(nu=384, ni=384)


def _new_part(n_users=True):
    lad = _lad()
    full = DeviceCSC.from_host(lad.g)
    full.n_users = lad.nu if n_users else None
    part = GraphPart(full, 1, 0)
    part.build_bins()
    return part


@functools.lru_cache(maxsize=None)
def _part():
    """Shared read-only partition (engines never modify it)."""
    return _new_part()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel()).cuda()


def _als_env(monkeypatch, mode):
    """0: fp32 everywhere; "bf16": bf16 for fused rows too; "default": fp32
    fused rows + bf16 hub chunks; "gather": LUX_ALS_BF_GATHER on top of the
    default (not extended past K = 64)."""
    for k in ("LUX_ALS_F32", "LUX_ALS_BF16", "LUX_ALS_BF_GATHER"):
        monkeypatch.delenv(k, raising=False)
    if mode == 0:
        monkeypatch.setenv("LUX_ALS_F32", "1")
    elif mode == "bf16":
        monkeypatch.setenv("LUX_ALS_BF16", "1")
    elif mode == "gather":
        monkeypatch.setenv("LUX_ALS_BF_GATHER", "1")
    else:
        assert mode in (1, "default")


def _check_phase(basis, before, after, lo, hi, K, tol_row, tol_hub):
    """Residual contract on rows [lo, hi); deg-0 rows there, and every row
    outside, keep their vector bit for bit."""
    lad = _lad()
    worst = 0.0
    for v in range(lo, hi):
        d = lad.degs[v]
        if d == 0:
            assert np.array_equal(after[v], before[v]), f"deg-0 row {v}"
            continue
        worst = max(worst, _phase_residual(
            lad.g, basis, after, v, v + 1, K,
            tol_hub if d >= dl.T2 else tol_row))
    outside = np.ones(lad.g.nv, bool)
    outside[lo:hi] = False
    assert np.array_equal(after[outside], before[outside])
    return worst


def _assert_two_sided_hubs(eng):
    lad, p = _lad(), eng.part
    assert eng.nbigu > 0 and p.nbig > eng.nbigu
    b2v = eng.bin2vs.cpu().numpy()
    want_u = np.nonzero(lad.degs[:lad.nu] >= dl.T2)[0]
    want_i = lad.nu + np.nonzero(lad.degs[lad.nu:] >= dl.T2)[0]
    assert sorted(b2v[:eng.nbigu]) == list(want_u)
    assert sorted(b2v[eng.nbigu:p.nbig]) == list(want_i)


def _two_phases(eng, K, init, tol_row, tol_hub):
    lad = _lad()
    nu, nv = lad.nu, lad.g.nv
    eng.old.copy_(_dev(init))
    eng.half_step("users")
    got_u = eng.vectors().cpu().numpy().copy()
    wu = _check_phase(init, init, got_u, 0, nu, K, tol_row, tol_hub)
    eng.half_step("items")
    got_i = eng.vectors().cpu().numpy().copy()
    wi = _check_phase(got_u, got_u, got_i, nu, nv, K, tol_row, tol_hub)
    print(f"K={K}: worst residual users {wu:.3g} items {wi:.3g}")


# 1 ------------------------------------------------------------------------

@pytest.mark.parametrize("K", [65, 96, 127, 128])
def test_wide_residual_ladder(K, monkeypatch):
    """Exact-fp32 ALS over the whole ladder on BOTH sides: fused rows to
    5e-5, hub rows to 2e-4. The item basis is the engine's own user
    output; user hubs make nbigu > 0, so the item phase runs on gram/rhs
    pointers offset by nbigu * 128 * 128 and nbigu * 128."""
    _als_env(monkeypatch, 0)
    eng = CFALSEngine(_part(), K=K)
    _assert_two_sided_hubs(eng)
    assert eng.gram.numel() == eng.part.nbig * KP * KP
    assert eng.rhs_h.numel() == eng.part.nbig * KP
    _two_phases(eng, K, _rand_init(_lad().g.nv, K, seed=42), F32_TOL,
                HUB_TOL)


# 2 ------------------------------------------------------------------------

def test_wide_jacobi_fallback(monkeypatch):
    """Without the bipartite boundary every row is solved from the old
    factors in one launch (absolute hubidx slots)."""
    K = 128
    _als_env(monkeypatch, 0)
    lad = _lad()
    part = _new_part(n_users=False)
    assert part.n_users is None
    eng = CFALSEngine(part, K=K)
    assert eng.lb is None and part.nbig == 2 * len(dl.LADDER_CHUNK)
    init = _rand_init(lad.g.nv, K, seed=43)
    eng.old.copy_(_dev(init))
    eng.step()
    got = eng.vectors().cpu().numpy()
    _check_phase(init, init, got, 0, lad.g.nv, K, F32_TOL, HUB_TOL)


# 3 ------------------------------------------------------------------------

def _hub_gram_ref128(g, v, F):
    """int64 upper-triangular 128x128 Gram S^T S and rhs S^T w of row v for
    integer-valued factors F (dims >= K are zero padding)."""
    b = 0 if v == 0 else int(g.col_end[v - 1])
    e = int(g.col_end[v])
    K = F.shape[1]
    S = np.asarray(F, np.float64)[g.src[b:e]]  # ints: f64 matmul is exact
    G = np.zeros((KP, KP), np.int64)
    G[:K, :K] = np.rint(S.T @ S).astype(np.int64)
    rhs = np.zeros(KP, np.int64)
    rhs[:K] = np.rint(S.T @ g.weight[b:e].astype(np.float64))
    return np.triu(G), rhs


@functools.lru_cache(maxsize=None)
def _gram_ref(K):
    lad = _lad()
    F = dl.int_factors(lad.g.nv, K)
    hubs = np.nonzero(lad.degs >= dl.T2)[0]
    return F, {int(v): _hub_gram_ref128(lad.g, int(v), F) for v in hubs}


def _check_hub_slots(eng, lo, hi, base, refs, K):
    p = eng.part
    b2v = eng.bin2vs.cpu().numpy()
    hubidx = eng.hubidx.cpu().numpy()
    gram = eng.gram.cpu().numpy().reshape(p.nbig, KP, KP)
    rhs = eng.rhs_h.cpu().numpy().reshape(p.nbig, KP)
    for i in range(lo, hi):
        v = int(b2v[i])
        assert hubidx[v] == i - base
        G, r = refs[v]
        deg = _lad().degs[v]
        # the lower triangle is never written; np.triu only selects
        assert not np.tril(gram[i], -1).any()
        assert np.array_equal(np.triu(gram[i]).astype(np.int64), G), \
            f"hub {v} degree {deg}: Gram differs"
        assert np.array_equal(gram[i], gram[i].round())
        assert not gram[i][K:].any() and not gram[i][:, K:].any()
        assert np.array_equal(rhs[i].astype(np.int64), r) \
            and np.array_equal(rhs[i], rhs[i].round()), \
            f"hub {v} degree {deg}: rhs differs"
        assert not rhs[i][K:].any()
    return gram, rhs


@pytest.mark.parametrize("K", [80, 128])
@pytest.mark.parametrize("mode", [0, 1])
def test_wide_hub_gram_exact(mode, K, monkeypatch):
    """Integer factors 0..6 (exact in bf16 too; 36*24577 < 2^24): every hub
    slot's Gram upper triangle and rhs must EQUAL the int64 S^T S and
    S^T w in both chunk modes, entries with row or column >= K zero. No
    tolerance: this pins the 8x8 tile -> accumulator map and the wave-1
    block permutation, both MFMA lane maps, and every chunk tail, on user
    hubs (slots [0, nbigu)) and item hubs (offset base)."""
    _als_env(monkeypatch, mode)
    eng = CFALSEngine(_part(), K=K)
    assert eng.old_bf is None
    _assert_two_sided_hubs(eng)
    nbigu, nbig = eng.nbigu, eng.part.nbig
    F, refs = _gram_ref(K)
    eng.old.copy_(_dev(F))
    eng.half_step("users")
    gram_u, rhs_u = _check_hub_slots(eng, 0, nbigu, 0, refs, K)
    assert not gram_u[nbigu:].any() and not rhs_u[nbigu:].any()
    eng.old.copy_(_dev(F))  # items read the same integer table
    eng.half_step("items")
    gram_i, rhs_i = _check_hub_slots(eng, nbigu, nbig, nbigu, refs, K)
    # the item phase left the user hubs' scratch alone
    assert np.array_equal(gram_i[:nbigu], gram_u[:nbigu])
    assert np.array_equal(rhs_i[:nbigu], rhs_u[:nbigu])


# 4 ------------------------------------------------------------------------

@pytest.mark.parametrize("mode,K", [("bf16", 65), ("bf16", 128),
                                    ("default", 128), ("gather", 128)])
def test_wide_bf16_ladder(mode, K, monkeypatch):
    """bf16 Gram at the project's bf16 tolerance: forced onto the fused
    rows too, the default (bf16 hub chunks only), and with
    LUX_ALS_BF_GATHER set, which allocates no replica above K = 64."""
    _als_env(monkeypatch, mode)
    eng = CFALSEngine(_part(), K=K)
    assert eng.old_bf is None
    _two_phases(eng, K, _rand_init(_lad().g.nv, K, seed=44), BF16_TOL,
                BF16_TOL)


# 5 ------------------------------------------------------------------------

def test_wide_multipart_single_process(monkeypatch):
    """Two partitions stepped phase-locked in one process at K = 96: each
    phase meets the residual contract against the synced basis the
    partitions read; replicas agree exactly after the final sync."""
    monkeypatch.setenv("LUX_ALS_F32", "1")
    nu, ni, ne, K = 1000, 256, 40000, 96
    full = DeviceCSC.bipartite(nu, ni, ne, seed=19)
    pa = GraphPart(full, 2, 0, keep_full=True)
    pb = GraphPart(full, 2, 1)
    ea, eb = CFALSEngine(pa, K=K), CFALSEngine(pb, K=K)
    g = Graph.bipartite(nu, ni, ne, seed=19)
    init = _rand_init(pa.nv, K, seed=77)
    for e in (ea, eb):
        e.old.copy_(torch.from_numpy(init.ravel()))
    for _ in range(2):
        for ph, (lo, hi) in (("users", (0, nu)), ("items", (nu, pa.nv))):
            basis = ea.vectors().cpu().numpy().copy()
            ea.half_step(ph)
            eb.half_step(ph)
            _sync_parts((ea, eb), K)
            cur = ea.vectors().cpu().numpy()
            _phase_residual(g, basis, cur, lo, hi, K, F32_TOL)
    np.testing.assert_array_equal(ea.vectors().cpu().numpy(),
                                  eb.vectors().cpu().numpy())


# 6 ------------------------------------------------------------------------

def test_wide_default_sweeps_beat_sgd(monkeypatch):
    """Three default-mode ALS sweeps at K = 128 stay finite and reach a
    lower loss than three SGD sweeps."""
    _als_env(monkeypatch, "default")
    nu, ni, ne, K = 5000, 512, 200000, 128
    full = DeviceCSC.bipartite(nu, ni, ne, seed=9)
    g = Graph.bipartite(nu, ni, ne, seed=9)
    sgd = CFEngine(GraphPart(full, 1, 0, keep_full=True), K=K)
    als = CFALSEngine(GraphPart(full, 1, 0), K=K)
    for _ in range(3):
        sgd.step()
        als.step()
    va = als.vectors().cpu().numpy()
    assert np.isfinite(va).all()
    l_als = cpu_ref.cf_loss(g, K, va)
    l_sgd = cpu_ref.cf_loss(g, K, sgd.vectors().cpu().numpy())
    assert np.isfinite(l_als) and l_als < l_sgd


# 7 ------------------------------------------------------------------------

NATIVE_NU, NATIVE_NI, NATIVE_NE = 4000, 128, 640000


@pytest.fixture(scope="module")
def native_graph(tmp_path_factory):
    """4000 users x 128 items, 320000 ratings stored both ways: item rows
    (degree ~2500) are hubs, so the native runtime's 128-pitch scratch, the
    hub chunk and the hub solve kernels run; user rows (degree ~80) run the
    fused kernel. 128 items and 4000 users keep every Gram as full-rank as
    its degree allows."""
    lux = str(tmp_path_factory.mktemp("k128") / "b.lux")
    r = subprocess.run([f"{BIN}/rmat_gen", "-kind", "bipartite", "-users",
                        str(NATIVE_NU), "-items", str(NATIVE_NI), "-ne",
                        str(NATIVE_NE), "-o", lux], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return lux, Graph.load(lux, want_weights=True)


@pytest.mark.parametrize("multi", [False, True])
def test_wide_native_one_sweep(native_graph, tmp_path, multi):
    """bin/col_filter -als -k 128, one alternating sweep from the native
    init (als_init is its Python twin): user rows satisfy their normal
    equations over the init, item rows over the dumped user rows, to 5e-5
    (exact-fp32 Gram; the default would run the item hubs in bf16). Once
    more through the native multi-GPU worker at world 1."""
    lux, g = native_graph
    K = 128
    out = str(tmp_path / "v.luxs")
    env = dict(os.environ, LUX_ALS_F32="1")
    env.pop("LUX_ALS_BF16", None)
    if multi:
        env["LUX_NATIVE_MULTI"] = "1"
    r = subprocess.run([f"{BIN}/col_filter", "-file", lux, "-als", "-k",
                        str(K), "-users", str(NATIVE_NU), "-ni", "1",
                        "-dump", out], cwd=ROOT, capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got, it = ck.load_state(out)
    assert it == 1 and got.shape == (g.nv, K)
    degs = np.diff(np.concatenate([[0], g.col_end.astype(np.int64)]))
    assert (degs[NATIVE_NU:] >= dl.T2).any() and (degs[:NATIVE_NU] > 0).any()
    init = als_init(g.nv, K).reshape(g.nv, K)
    wu = _phase_residual(g, init, got, 0, NATIVE_NU, K, F32_TOL)
    mid = init.copy()
    mid[:NATIVE_NU] = got[:NATIVE_NU]
    wi = _phase_residual(g, mid, got, NATIVE_NU, g.nv, K, F32_TOL)
    print(f"native multi={multi}: worst residual users {wu:.3g} "
          f"items {wi:.3g}")
    z = degs == 0
    assert np.array_equal(got[z], init[z])


def test_wide_native_rejects_k129(native_graph):
    lux, _ = native_graph
    r = subprocess.run([f"{BIN}/col_filter", "-file", lux, "-als", "-k",
                        "129", "-users", str(NATIVE_NU), "-ni", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "128" in r.stdout + r.stderr


# 8 ------------------------------------------------------------------------

def test_wide_python_rejects_k129():
    with pytest.raises(AssertionError, match="128"):
        CFALSEngine(_part(), K=129)
