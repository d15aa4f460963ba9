"""Community detection app driver (no reference equivalent): the Louvain
method, one colour class of the greedy colouring (-order degree | id | hash)
at a time, on the underlying simple undirected graph of -file / -synthetic.
-weighted sums the edge weights over all occurrences of an edge (-file with
weights, or -synthetic rmat:... with endpoint-hash weights in [1, -wmax]).
-ni MAX_SWEEPS bounds the sweeps of a level, -levels MAX_LEVELS the levels
(default: run out). Single GPU."""
import sys

from .. import dist as dx
from ..colouring_engine import ORDERS
from ..louvain_engine import LouvainEngine
from .common import (ElapsedTimer, attach_hash_weights, load_part,
                     parse_input_args, print_memory_estimate)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    max_levels = 0
    if "-levels" in argv:
        i = argv.index("-levels")
        max_levels = int(argv[i + 1])
        del argv[i:i + 2]
    a = parse_input_args(argv)
    max_sweeps = a.num_iter if "-ni" in argv else 0
    if a.order not in ORDERS:
        raise SystemExit(f"-order must be one of {', '.join(ORDERS)} "
                         f"(got {a.order!r})")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("louvain is single-GPU for now: a class reads its "
                         "neighbours' communities on one device (run with "
                         "one process)")
    import time
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    try:
        part = load_part(a, device, weighted=a.weighted and bool(a.file))
    except IOError as e:
        raise SystemExit(f"louvain -weighted needs edge weights: {e}")
    if a.weighted and not a.file:
        attach_hash_weights(a, part)
    # the sorted records and the weighted adjacency (three words per entry),
    # the colouring's rows while it runs, and the per-vertex state
    print_memory_estimate(part.nv, part.ne, 1, weighted=a.weighted, k=6)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        eng = LouvainEngine(part, order=a.order, weighted=a.weighted)
    except ValueError as e:
        raise SystemExit(f"louvain: {e}")
    torch.cuda.synchronize()
    prep = time.perf_counter() - t0
    eng.timed = True
    with ElapsedTimer():
        eng.solve(max_sweeps=max_sweeps, max_levels=max_levels)
    st, ph = eng.stats, eng.phase_ms
    per_level = ",".join(str(t[2]) for t in eng.level_trace)
    print(f"[lux] louvain: {eng.num_communities()} communities, modularity "
          f"{eng.modularity():.6f} (Qnum {eng.qnum()}, W {st['W']}), levels "
          f"{st['levels']}, sweeps {st['sweeps']} ({per_level}), "
          f"{st['colours']} colours at level 0 in {a.order} order")
    print(f"[lux] louvain: launches {st['launches']} ({st['fused_classes']} "
          f"classes fused), hub rows {st['hub_rows']} ({st['hub_items']} "
          f"items), host reads {st['host_reads']}, preparation {prep:.3f} s, "
          f"phases orient/adjacency/colour/plan/move/aggregate = "
          f"{ph['orient']:.3f}/{ph['adjacency']:.3f}/{ph['colour']:.3f}/"
          f"{ph['plan']:.3f}/{ph['move']:.3f}/{ph['aggregate']:.3f} ms")
    if a.verbose:
        print("level,sweep,moved,qnum")
        for row in eng.sweep_trace:
            print("%d,%d,%d,%d" % row)
    if a.check:
        if max_levels and st["levels"] >= max_levels and \
                eng.level_trace[-1][3]:
            print("[lux] -check skipped: the solve was cut by -levels")
        else:
            mistakes = eng.check()
            tag = "PASS" if mistakes == 0 else "FAIL"
            print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
