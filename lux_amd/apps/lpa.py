"""Community detection app driver (no reference equivalent): label
propagation, one colour class of the greedy colouring (-order degree | id |
hash) at a time, on the underlying simple undirected graph of -file /
-synthetic. -ni MAX_SWEEPS stops early (default: run to convergence).
Single GPU."""
import sys

from .. import dist as dx
from ..colouring_engine import ORDERS
from ..lpa_engine import LPAEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse_input_args(argv)
    max_sweeps = a.num_iter if "-ni" in argv else 0
    if a.order not in ORDERS:
        raise SystemExit(f"-order must be one of {', '.join(ORDERS)} "
                         f"(got {a.order!r})")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("lpa is single-GPU for now: a class reads its "
                         "neighbours' labels on one device (run with one "
                         "process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # oriented copy + full adjacency (two words per edge), the colouring's
    # rows while it runs, and the per-vertex state
    print_memory_estimate(part.nv, part.ne, 1, k=4)
    eng = LPAEngine(part, order=a.order)  # preparation
    eng.timed = True
    with ElapsedTimer():
        eng.solve(max_sweeps=max_sweeps)
    st, ph = eng.stats, eng.phase_ms
    sizes = eng.sizes()
    big = int(sizes.argmax().item()) if part.nv else 0
    print(f"[lux] lpa: {eng.num_communities()} communities, largest "
          f"(label {big}, size {int(sizes[big].item()) if part.nv else 0}), "
          f"intra edges {eng.intra_edges()} of {st['simple_edges']}, "
          f"modularity {eng.modularity():.6f}, {st['colours']} colours in "
          f"{a.order} order, sweeps {st['sweeps']}"
          f"{'' if eng.converged() else ' (not converged)'}, launches per "
          f"sweep {st['launches']} ({st['fused_classes']} classes fused), "
          f"hub rows {st['hub_rows']} ({st['hub_items']} items), host reads "
          f"{st['host_reads']}, phases orient/adjacency/colour/plan/solve = "
          f"{ph['orient']:.3f}/{ph['adjacency']:.3f}/{ph['colour']:.3f}/"
          f"{ph['plan']:.3f}/{ph['solve']:.3f} ms")
    if a.verbose:
        print("sweep,evaluated,changed")
        for row in eng.sweep_trace:
            print("%d,%d,%d" % row)
    if a.check:
        if eng.converged():
            mistakes = eng.check()
            tag = "PASS" if mistakes == 0 else "FAIL"
            print(f"[{tag}] {mistakes} mistakes")
        else:
            print("[lux] -check skipped: the solve did not converge")
    return eng


if __name__ == "__main__":
    main()
