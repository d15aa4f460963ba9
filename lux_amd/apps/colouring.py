"""Graph colouring / maximal independent set app driver (no reference
equivalent): the greedy colouring in priority order (-order degree | id |
hash) of the underlying simple undirected graph of -file / -synthetic; the
class of colour 0 is the lexicographically first maximal independent set.
Single GPU."""
import sys

from .. import dist as dx
from ..colouring_engine import ORDERS, ColouringEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    if a.order not in ORDERS:
        raise SystemExit(f"-order must be one of {', '.join(ORDERS)} "
                         f"(got {a.order!r})")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("colouring is single-GPU for now: a round notifies "
                         "successors on one device (run with one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # oriented copy + predecessor and successor rows (two words per edge)
    # and the sort keys while the first is built
    print_memory_estimate(part.nv, part.ne, 1, k=4)
    eng = ColouringEngine(part, order=a.order)  # preparation: orient + split
    eng.timed = True
    with ElapsedTimer():
        eng.solve()
    st, ph = eng.stats, eng.phase_ms
    sizes = eng.class_sizes()
    print(f"[lux] colouring: {eng.num_colours()} colours in {a.order} order, "
          f"MIS {int(sizes[0].item()) if sizes.numel() else 0} vertices, "
          f"largest class "
          f"{int(sizes.max().item()) if sizes.numel() else 0}, "
          f"{st['simple_edges']} simple edges, max degree "
          f"{st['max_degree']}, max predecessor row {st['max_pred']}, "
          f"rounds {st['rounds']} ({st['fused_rounds']} fused), launches "
          f"{st['launches']}, host reads {st['host_reads']}, phases "
          f"orient/split/solve = {ph['orient']:.3f}/{ph['split']:.3f}/"
          f"{ph['solve']:.3f} ms")
    if a.verbose:
        from ..trace import IterTrace
        tr = IterTrace()
        for rnd, coloured in eng.round_trace:
            tr.record(round=rnd, coloured=coloured)
        print(tr.to_csv(), end="")
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
