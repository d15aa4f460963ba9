"""Implicit-feedback ALS on the CPU: the numpy oracle against the equations
of API.md written out densely, and the CLI flags."""
import numpy as np

from lux_amd import cpu_ref
from lux_amd.apps.common import parse_input_args
from lux_amd.graph import Graph

NU, NI, K, ALPHA, REG = 6, 5, 3, 2.0, 0.1
# (user, item id, weight): user 1 saw item 7 twice (a parallel entry), user 4
# and item 10 have no entry at all; every rating is stored both ways
RATINGS = [(0, 6, 1), (0, 8, 3), (1, 7, 2), (1, 7, 5), (2, 6, 4), (2, 9, 1),
           (3, 8, 2), (3, 9, 0), (5, 6, 1), (5, 7, 3), (5, 9, 2)]


def _graph():
    e = np.array(RATINGS)
    src = np.concatenate([e[:, 1], e[:, 0]]).astype(np.uint32)
    dst = np.concatenate([e[:, 0], e[:, 1]]).astype(np.uint32)
    w = np.concatenate([e[:, 2], e[:, 2]]).astype(np.int32)
    return Graph.from_edges(NU + NI, src, dst, w)


def _dense_phase(vec, rows, other):
    """Solve `rows` against `other` from the dense count / weight tables."""
    n = NU + NI
    cnt, wsum = np.zeros((n, n)), np.zeros((n, n))
    for u, i, w in RATINGS:
        for a, b in ((u, i), (i, u)):
            cnt[a, b] += 1
            wsum[a, b] += w
    Y = vec[other]
    out = vec.copy()
    for v in rows:
        A = Y.T @ Y + ALPHA * (Y.T * wsum[v, other]) @ Y + REG * np.eye(K)
        b = (cnt[v, other] + ALPHA * wsum[v, other]) @ Y
        out[v] = np.linalg.solve(A, b)
    return out


def test_cf_ials_matches_dense_equations():
    g = _graph()
    init = np.random.default_rng(3).standard_normal((NU + NI, K))
    users, items = np.arange(NU), np.arange(NU, NU + NI)
    want = _dense_phase(init, users, items)
    want = _dense_phase(want, items, users)
    got = cpu_ref.cf_ials(g, K, 1, ALPHA, REG, init, NU)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)
    assert not got[4].any() and not got[10].any()  # the zero-entry rows
    assert got[[0, 1, 2, 3, 5]].any(1).all()
    # a further sweep is an exact minimisation per phase: the loss drops
    l1 = cpu_ref.cf_ials_loss(g, K, got, ALPHA, REG, NU)
    l2 = cpu_ref.cf_ials_loss(
        g, K, cpu_ref.cf_ials(g, K, 1, ALPHA, REG, got, NU), ALPHA, REG, NU)
    assert l2 < l1 < cpu_ref.cf_ials_loss(g, K, init, ALPHA, REG, NU)


def test_parse_implicit_flags():
    a = parse_input_args(["-als", "-implicit", "-alpha", "2.5", "-reg", "0.1"])
    assert a.als and a.implicit and a.alpha == 2.5 and a.reg == 0.1
    d = parse_input_args(["-als"])
    assert not d.implicit and d.alpha == 40.0 and d.reg == 0.01
