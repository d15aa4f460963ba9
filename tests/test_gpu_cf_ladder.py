"""CF kernels (cf.hip SGD, cf_als.hip ALS) on the two-sided degree ladder.

The value tests in test_gpu_cf.py compare factors after a few sweeps at a
step size of 3.5e-7 from a constant init: almost every row ends within
tolerance of where it started, so they cannot tell a working kernel from a
skipped one. Here the SGD kernels sweep into a ZEROED output, so newv/gamma
is the accumulated gradient at full fp32 precision, every vertex holds a
distinct vector, and both sides of the bipartite graph carry every degree
at which a kernel, a tile loop or a chunk loop changes path
(tests/degree_ladder.py). Hub-row edge coverage uses integer inputs on
which fp32 is exact.

Which case reaches which kernel (K, LUX_CF_TILE, ladder degree):
  cf_wave_kernel        degrees 1..31 at every K; 32..2047 at K > 64
  cf_tile_kernel<32|64> degrees 32..2047 at K <= 64; the static K == 64
                        full-tile pass from degree 32|64 up, the generic
                        pass for K < 64 and for every ragged tail
  cf_tile_chunk_kernel<32|64>  degrees >= 2048 at K <= 64 (K < 64 included)
  cf_chunk_kernel       degrees >= 2048 at K in {65, 128, 255, 256}
  cf_als_solve_kernel<0|1|2>   degrees 1..2047
  cf_als_gram_chunk_kernel<0|1|2> + cf_als_hub_solve_kernel  degrees >= 2048
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import degree_ladder as dl  # noqa: E402
from test_gpu_cf import _phase_residual, _rand_init  # noqa: E402

from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd.cf_engine import CFALSEngine, CFEngine  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402

GAMMA = dl.CF_GAMMA


@functools.lru_cache(maxsize=None)
def _lad():
    return dl.bipartite_ladder()


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


def _set_tile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("LUX_CF_TILE", raising=False)
    else:
        monkeypatch.setenv("LUX_CF_TILE", str(tile))


def _als_env(monkeypatch, mode):
    """ALS Gram mode of the hub chunks: 0 exact fp32, 1 bf16 MFMA with fp32
    gathers (the default), 2 bf16 MFMA with dword-pair bf16 gathers (also
    switches the fused rows to their mode-2 kernel)."""
    for k in ("LUX_ALS_F32", "LUX_ALS_BF16", "LUX_ALS_BF_GATHER"):
        monkeypatch.delenv(k, raising=False)
    if mode == 0:
        monkeypatch.setenv("LUX_ALS_F32", "1")
    elif mode == "bf16":  # mode 1 for the fused rows as well
        monkeypatch.setenv("LUX_ALS_BF16", "1")
    elif mode == 2:
        monkeypatch.setenv("LUX_ALS_BF_GATHER", "1")


def _sweep(K, old_np):
    """One lux_gpu_cf_iter into a zeroed newv; returns raw gamma*acc."""
    p = _part()
    old = _dev(old_np)
    new = torch.zeros(p.vp * K, dtype=torch.float32, device="cuda")
    ng.cf_iter(torch.cuda.current_stream().cuda_stream, p.n0, p.bin0, p.n1,
               p.bin1, p.n2, p.bin2, p.nbig, p.bin2v, p.row_ptr, p.col,
               p.weight, old, new, p.row_left, K)
    torch.cuda.synchronize()
    return new.cpu().numpy().reshape(p.vp, K)


def test_ladder_bins():
    """The device bins hold exactly the rows the ladder puts there."""
    lad, p = _lad(), _part()
    d = lad.degs
    assert p.vp == lad.g.nv and p.ep == lad.g.ne
    assert p.n0 == ((d > 0) & (d < dl.T1)).sum()
    assert p.n1 == ((d >= dl.T1) & (d < dl.T2)).sum()
    assert p.nbig == (d >= dl.T2).sum() == 2 * len(dl.LADDER_CHUNK)
    assert p.n2 == (-(-d[d >= dl.T2] // dl.CHUNK_EDGES)).sum()
    assert np.array_equal(p.col.cpu().numpy().view(np.uint32), lad.g.src)


# ------------------------------------------------------------- SGD ----------

TILE_KS = [1, 3, 4, 20, 63, 64]     # LDS-tiled path, both tile sizes
WAVE_KS = [65, 128, 255, 256]       # cf_wave_kernel + cf_chunk_kernel
SGD_CASES = [(K, t) for K in TILE_KS for t in (32, 64)] \
    + [(K, None) for K in WAVE_KS]


@functools.lru_cache(maxsize=None)
def _exact_ref(K, side):
    lad = _lad()
    F = dl.int_factors(lad.g.nv, K)
    if side == "users":
        F[:lad.nu] = 0
    else:
        F[lad.nu:] = 0
    acc, _ = dl.sgd_gradient_ref(lad.g, F)
    return F, acc


@functools.lru_cache(maxsize=None)
def _rand_ref(K):
    lad = _lad()
    old = _rand_init(lad.g.nv, K, seed=100 + K)
    acc, scale = dl.sgd_gradient_ref(lad.g, old)
    return old, acc, scale


@pytest.mark.parametrize("side", ["users", "items"])
@pytest.mark.parametrize("K,tile", SGD_CASES)
def test_sgd_gradient_exact(K, tile, side, monkeypatch):
    """Exact regime: dst vectors zero (err = w exactly), src vectors small
    integers distinct per vertex and dimension. Every partial sum is an
    integer below 2^24, exact in fp32 in any order, so the only rounding
    is the gamma multiply and up to 4 chunk atomics (< 2.4e-7 relative);
    the bound 1e-6 is below one dropped or doubled weight-1 edge at degree
    24577 (>= 8e-6). The other side reads all-zero sources: exactly 0."""
    _set_tile(monkeypatch, tile)
    lad = _lad()
    F, acc = _exact_ref(K, side)
    raw = _sweep(K, F)
    mine = slice(0, lad.nu) if side == "users" else slice(lad.nu, None)
    other = slice(lad.nu, None) if side == "users" else slice(0, lad.nu)
    got = raw.astype(np.float64) / GAMMA
    bad = dl.sgd_exact_bad_rows(got[mine], acc[mine])
    assert len(bad) == 0, (
        f"rows {bad[:8]} degrees {lad.degs[mine][bad[:8]]}: "
        f"{got[mine][bad[:2]]} != {acc[mine][bad[:2]]}")
    assert not raw[other].any()
    assert not raw[lad.degs == 0].any()


@pytest.mark.parametrize("K,tile", SGD_CASES)
def test_sgd_gradient_random(K, tile, monkeypatch):
    """Random regime (0.1*N(0,1)+0.1 factors) against the f64 gradient:
    |newv/gamma - acc|_k <= 1e-4 * A_k with A_k = sum_e |err_e||s_ek|.
    Sequential fp32 accumulation of the degree-24577 row errs by 4.8e-6*A
    (tests/test_degree_ladder.py re-measures it); a skipped row or a
    gather from the wrong source is off by a large fraction of A."""
    _set_tile(monkeypatch, tile)
    lad = _lad()
    old, acc, scale = _rand_ref(K)
    raw = _sweep(K, old)
    got = raw.astype(np.float64) / GAMMA
    # the bound itself must reject a kernel that did nothing
    nonempty = np.nonzero(lad.degs > 0)[0]
    assert np.array_equal(
        dl.sgd_rand_bad_rows(np.zeros_like(acc), acc, scale), nonempty)
    bad = dl.sgd_rand_bad_rows(got, acc, scale)
    assert len(bad) == 0, (
        f"rows {bad[:8]} degrees {lad.degs[bad[:8]]}: worst "
        f"{(np.abs(got - acc)[bad] / scale[bad]).max():.3g} * A")
    assert not raw[lad.degs == 0].any()


@pytest.mark.parametrize("K", [64, 128])
def test_sgd_engine_step_gradient(K, monkeypatch):
    """CFEngine.step() end to end: (new - old*(1 - gamma*lambda)) / gamma
    against the same f64 gradient. RESTRICTED to rows of degree >= 32:
    new is old plus a ~1e-6 relative increment, so the subtraction cancels
    to the rounding of old and new themselves, and below the wave bin that
    rounding is as large as the gradient. Bound per component, all from
    the reference side:
      1e-4 * A_k                     the kernel bound of the tests above
      + 6 * 2^-24 * (|old_k| + gamma*A_k) / gamma
                                     one rounding of the seed old*(1 -
                                     gamma*lambda) (this also covers the
                                     factor itself rounding to 1.0f), one
                                     of the final add, up to 4 chunk
                                     atomics, each at most 2^-24 of
                                     |new_k| <= |old_k| + gamma*A_k.
    At degree 32 the second term is ~3% of A; a no-op is off by >= 30%."""
    _set_tile(monkeypatch, None)
    lad = _lad()
    old, acc, scale = _rand_ref(K)
    eng = CFEngine(_part(), K=K)
    eng.old.copy_(_dev(old))
    eng.step()
    new = eng.vectors().cpu().numpy().astype(np.float64)
    o = old.astype(np.float64)
    got = (new - o * (1.0 - GAMMA * dl.CF_LAMBDA)) / GAMMA
    bound = 1e-4 * scale + 6 * 2.0 ** -24 * (np.abs(o) + GAMMA * scale) \
        / GAMMA
    rows = np.nonzero(lad.degs >= dl.T1)[0]
    # the bound rejects a step that added nothing, on every checked row
    assert (np.abs(acc[rows]) > bound[rows]).any(1).all()
    err = np.abs(got - acc)
    badr = rows[(err[rows] > bound[rows]).any(1)]
    assert len(badr) == 0, f"rows {badr[:8]} degrees {lad.degs[badr[:8]]}"
    # rows with no in-edges: only the regulariser seed, bit-exact
    z = lad.degs == 0
    assert np.array_equal(
        eng.vectors().cpu().numpy()[z],
        (o[z] * (1.0 - GAMMA * dl.CF_LAMBDA)).astype(np.float32))


# ------------------------------------------------------------- ALS ----------

F32_TOL, HUB_TOL, BF16_TOL = 5e-5, 2e-4, 5e-2  # the project's tolerances


def _check_phase(basis, before, after, lo, hi, K, tol_row, tol_hub):
    """Residual contract on rows [lo, hi); deg-0 rows there, and every row
    outside, keep their vector bit for bit."""
    lad = _lad()
    for v in range(lo, hi):
        d = lad.degs[v]
        if d == 0:
            assert np.array_equal(after[v], before[v]), f"deg-0 row {v}"
            continue
        _phase_residual(lad.g, basis, after, v, v + 1, K,
                        tol_hub if d >= dl.T2 else tol_row)
    outside = np.ones(lad.g.nv, bool)
    outside[lo:hi] = False
    assert np.array_equal(after[outside], before[outside])


def _assert_two_sided_hubs(eng):
    lad, p = _lad(), eng.part
    assert eng.nbigu > 0 and p.nbig > eng.nbigu
    b2v = eng.bin2vs.cpu().numpy()
    want_u = np.nonzero(lad.degs[:lad.nu] >= dl.T2)[0]
    want_i = lad.nu + np.nonzero(lad.degs[lad.nu:] >= dl.T2)[0]
    assert sorted(b2v[:eng.nbigu]) == list(want_u)
    assert sorted(b2v[eng.nbigu:p.nbig]) == list(want_i)


@pytest.mark.parametrize("K", [1, 2, 17, 33, 63, 64])
def test_als_residual_ladder(K, monkeypatch):
    """Exact-fp32 ALS over the whole ladder on BOTH sides: fused rows to
    5e-5, hub rows (chunked Gram + hub solve) to 2e-4. User hubs make
    nbigu > 0, so the item phase runs on offset gram/rhs pointers and
    phase-relative hubidx slots. Each phase must leave the other side's
    rows (hub results included) untouched."""
    _als_env(monkeypatch, 0)
    lad = _lad()
    nu, nv = lad.nu, lad.g.nv
    eng = CFALSEngine(_part(), K=K)
    _assert_two_sided_hubs(eng)
    init = _rand_init(nv, K, seed=42)
    eng.old.copy_(_dev(init))
    eng.half_step("users")
    got_u = eng.vectors().cpu().numpy().copy()
    _check_phase(init, init, got_u, 0, nu, K, F32_TOL, HUB_TOL)
    eng.half_step("items")
    got_i = eng.vectors().cpu().numpy().copy()
    _check_phase(got_u, got_u, got_i, nu, nv, K, F32_TOL, HUB_TOL)


@pytest.mark.parametrize("K", [17, 64])
def test_als_jacobi_fallback_ladder(K, monkeypatch):
    """Without the bipartite boundary the engine solves every row from the
    old factors in one launch (absolute hubidx slots)."""
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


@pytest.mark.parametrize("mode,K", [(2, 2), (2, 20), (2, 64),
                                    ("bf16", 17), ("bf16", 64)])
def test_als_bf16_ladder(mode, K, monkeypatch):
    """bf16 Gram for fused AND hub rows at the project's bf16 residual
    tolerance: gather mode 2 (bf16 replica, dword-pair staging; even K)
    and, beside it, mode 1 forced onto the fused rows (LUX_ALS_BF16)."""
    _als_env(monkeypatch, mode)
    lad = _lad()
    nu, nv = lad.nu, lad.g.nv
    eng = CFALSEngine(_part(), K=K)
    assert (eng.old_bf is not None) == (mode == 2)
    init = _rand_init(nv, K, seed=44)
    eng.old.copy_(_dev(init))
    eng.half_step("users")
    got_u = eng.vectors().cpu().numpy().copy()
    _check_phase(init, init, got_u, 0, nu, K, BF16_TOL, BF16_TOL)
    eng.half_step("items")
    got_i = eng.vectors().cpu().numpy().copy()
    _check_phase(got_u, got_u, got_i, nu, nv, K, BF16_TOL, BF16_TOL)


@functools.lru_cache(maxsize=None)
def _gram_ref(K):
    lad = _lad()
    F = dl.int_factors(lad.g.nv, K)
    hubs = np.nonzero(lad.degs >= dl.T2)[0]
    return F, {int(v): dl.hub_gram_ref(lad.g, int(v), F) for v in hubs}


def _check_hub_slots(eng, lo, hi, base, refs):
    """Hub list entries [lo, hi) own scratch slots base + hubidx[v]; the
    upper triangle of each Gram and the rhs EQUAL the int64 references."""
    p = eng.part
    b2v = eng.bin2vs.cpu().numpy()
    hubidx = eng.hubidx.cpu().numpy()
    gram = eng.gram.cpu().numpy().reshape(p.nbig, 64, 64)
    rhs = eng.rhs_h.cpu().numpy().reshape(p.nbig, 64)
    for i in range(lo, hi):
        v = int(b2v[i])
        assert hubidx[v] == i - base
        G, r = refs[v]
        deg = _lad().degs[v]
        assert np.array_equal(np.triu(gram[i]).astype(np.int64), G), \
            f"hub {v} degree {deg}: Gram differs"
        assert np.array_equal(np.triu(gram[i]), np.triu(gram[i]).round())
        assert np.array_equal(rhs[i].astype(np.int64), r) \
            and np.array_equal(rhs[i], rhs[i].round()), \
            f"hub {v} degree {deg}: rhs differs"
    return gram, rhs


@pytest.mark.parametrize("K", [64, 20])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_als_hub_gram_exact(mode, K, monkeypatch):
    """Integer factors 0..6 (exact in bf16 too; 36*24577 < 2^24): every hub
    slot's Gram upper triangle and rhs must EQUAL the int64 S^T S and
    S^T w in all three chunk modes. No tolerance: this pins the 16x16x4
    and 16x16x32 lane maps, the transposed bf16 panel, the dword-pair
    staging and every chunk tail, on user hubs (slots [0, nbigu)) and item
    hubs (offset base, phase-relative slots)."""
    _als_env(monkeypatch, mode)
    eng = CFALSEngine(_part(), K=K)
    assert (eng.old_bf is not None) == (mode == 2)
    _assert_two_sided_hubs(eng)
    nbigu, nbig = eng.nbigu, eng.part.nbig
    F, refs = _gram_ref(K)
    eng.old.copy_(_dev(F))
    eng.half_step("users")
    gram_u, rhs_u = _check_hub_slots(eng, 0, nbigu, 0, refs)
    assert not gram_u[nbigu:].any() and not rhs_u[nbigu:].any()
    eng.old.copy_(_dev(F))  # items read the same integer table
    eng.half_step("items")
    gram_i, rhs_i = _check_hub_slots(eng, nbigu, nbig, nbigu, refs)
    # the item phase left the user hubs' scratch alone
    assert np.array_equal(gram_i[:nbigu], gram_u[:nbigu])
    assert np.array_equal(rhs_i[:nbigu], rhs_u[:nbigu])
