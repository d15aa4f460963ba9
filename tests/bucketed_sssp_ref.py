"""Plain-numpy reference for the bucketed (near-far delta-stepping) weighted
SSSP schedule (no GPU, no native code). It follows the engine's rules step
by step — the active set is the dirty vertices with label <= limit, an
empty active set advances the limit to the bucket of the smallest dirty
label, relaxation is Jacobi, a push keeps the deferred vertices dirty and a
pull replaces the dirty set by the changed one — and records what the
engine's per-iteration trace has to show.
"""
import numpy as np

import weighted_sssp_ref as ref

INF, SAT = ref.INF, ref.SAT


def first_limit(delta):
    return min(delta - 1, SAT)


def next_limit(m, delta):
    """Limit of the bucket that holds label m: empty buckets are skipped in
    one jump; the clamp keeps INF (never dirty) out of every bucket."""
    return min((m // delta + 1) * delta - 1, SAT)


def bucketed(g, source, delta, evol_div=8):
    """Bucketed min-plus relaxation from `source` over g.weight.

    Returns (labels u32, rows, advances, relaxed):
      rows      one (limit, active, volume, pull, deferred) per relaxing
                iteration: the limit it ran under, the size and summed
                out-degree of its active set, whether it was a dense pull
                sweep, and how many dirty vertices stayed beyond the limit
                once its result was classified (before any advance);
      advances  limit jumps (they relax nothing and are not iterations);
      relaxed   edges relaxed: the active set's out-edges on a push, every
                edge on a pull.
    The pull rule is weighted_sssp_ref.predict_pull's, applied to the
    active set; the seed's volume is not priced in the decision."""
    assert delta >= 1
    nv, ne = g.nv, g.ne
    src = g.src.astype(np.int64)
    dst = ref.edge_dst(g)
    w = np.asarray(g.weight, np.int32).view(np.uint32).astype(np.uint64)
    outdeg = np.bincount(src, minlength=nv)
    lab = np.full(nv, INF, np.uint64)
    lab[source] = 0
    dirty = np.zeros(nv, bool)
    dirty[source] = True
    limit = first_limit(delta)
    rows, advances, relaxed = [], 0, 0
    while True:
        assert len(rows) + advances <= 64 * nv + 64, "no fixed point"
        active = dirty & (lab <= np.uint64(limit))
        if not active.any():
            if not dirty.any():
                break
            limit = next_limit(int(lab[dirty].min()), delta)
            advances += 1
            continue
        n = int(active.sum())
        vol = int(outdeg[active].sum())
        priced = vol if rows else 0
        pull = bool(n > nv // 16 or priced > ne // evol_div)
        if pull:
            sel = lab[src] != np.uint64(INF)
            relaxed += ne
        else:
            sel = active[src]
            relaxed += vol
        cand = np.minimum(lab[src[sel]] + w[sel], np.uint64(SAT))
        new = lab.copy()
        np.minimum.at(new, dst[sel], cand)
        changed = new != lab
        dirty = changed if pull else ((dirty & ~active) | changed)
        lab = new
        deferred = int((dirty & (lab > np.uint64(limit))).sum())
        rows.append((limit, n, vol, pull, deferred))
    return lab.astype(np.uint32), rows, advances, relaxed
