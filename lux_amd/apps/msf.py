"""Minimum spanning forest app driver (no reference equivalent): the forest
of the underlying simple undirected graph of -file (a .lux file with
weights) or -synthetic rmat:... / rmat_folded:... (endpoint-hash weights in
[1, -wmax], as sssp -weighted), the weight of an edge being the minimum over
its occurrences. Single GPU."""
import sys

from .. import dist as dx
from ..msf_engine import MSFEngine
from .common import (ElapsedTimer, attach_hash_weights, load_part,
                     parse_input_args, print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("msf is single-GPU for now: a component's minimum "
                         "edge is searched over all its rows on one device "
                         "(run with one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    # -file: the loader raises on a file without weights
    try:
        part = load_part(a, device, weighted=bool(a.file))
    except IOError as e:
        raise SystemExit(f"msf needs edge weights: {e}")
    if not a.file:
        attach_hash_weights(a, part)
    # both directions of every simple edge with its id, and the edge list
    print_memory_estimate(part.nv, part.ne, 1, weighted=True, k=4)
    t0 = _clock(torch)
    eng = MSFEngine(part)  # preparation: orientation, weights, adjacency
    prep = _clock(torch) - t0
    eng.timed = True
    with ElapsedTimer():
        total = eng.solve()
    st, ph = eng.stats, eng.phase_ms
    print(f"[lux] msf: total weight {total}, {eng.num_edges()} forest edges "
          f"of {st['simple_edges']} simple edges, {eng.num_components()} "
          f"components")
    print(f"[lux] msf: rounds {st['rounds']} (scans {st['scans']}), scanned "
          f"{st['scanned']} entries, launches {st['launches']}, host reads "
          f"{st['host_reads']}, max degree {st['max_degree']}, hub rows "
          f"{st['hub_rows']} ({st['hub_items']} items), preparation "
          f"{prep:.3f} s, phases orient/weights/adjacency/solve = "
          f"{ph['orient']:.3f}/{ph['weights']:.3f}/{ph['adjacency']:.3f}/"
          f"{ph['solve']:.3f} ms")
    if a.verbose:
        print("round,components_with_edge,merged,scanned")
        for i, (cwe, merged, scanned) in enumerate(st["per_round"]):
            print(f"{i + 1},{cwe},{merged},{scanned}")
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


def _clock(torch):
    import time
    torch.cuda.synchronize()
    return time.perf_counter()


if __name__ == "__main__":
    main()
