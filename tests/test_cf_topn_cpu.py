"""cpu_ref.cf_topn, the numpy oracle of CFTopN, on a hand-worked example:
three users (vertices 0..2) and four items (3..6) with K = 2."""
import numpy as np

from lux_amd import cpu_ref

VEC = np.array([[1, 0], [0, 1], [1, 1],               # users
                [2, 1], [1, 2], [2, 1], [0, 0]], np.float32)  # items 3..6
INF = np.inf


def test_order_and_the_tie_rule():
    # scores: u0 = 2 1 2 0, u1 = 1 2 1 0, u2 = 3 3 3 0 over items 3..6
    items, scores = cpu_ref.cf_topn(VEC, [0, 1, 2], 3, 7, 3)
    assert items.dtype == np.int32 and scores.dtype == np.float64
    assert items.tolist() == [[3, 5, 4], [4, 3, 5], [3, 4, 5]]
    assert scores.tolist() == [[2, 2, 1], [2, 1, 1], [3, 3, 3]]


def test_exclusion_padding_and_duplicate_queries():
    ptr = np.array([0, 1, 4, 8, 8, 8, 8, 8])
    adj = np.array([3, 3, 4, 5, 3, 4, 5, 6])
    items, scores = cpu_ref.cf_topn(VEC, [0, 1, 2, 0], 3, 7, 3, ptr, adj)
    assert items.tolist() == [[5, 4, 6], [6, -1, -1], [-1, -1, -1],
                              [5, 4, 6]]
    assert scores.tolist() == [[2, 1, 0], [0, -INF, -INF],
                               [-INF, -INF, -INF], [2, 1, 0]]


def test_a_candidate_range_shorter_than_n():
    items, scores = cpu_ref.cf_topn(VEC, [2], 5, 7, 4)
    assert items.tolist() == [[5, 6, -1, -1]]
    assert scores.tolist() == [[3, 0, -INF, -INF]]
