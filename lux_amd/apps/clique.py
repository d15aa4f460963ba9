"""k-clique counting app driver (no reference equivalent): exact count of
the -clique K (3..8, default 4) cliques of the underlying simple undirected
graph of -file / -synthetic, oriented by -order degree (default) or id.
Single GPU."""
import sys

from .. import dist as dx
from ..clique_engine import K_MAX, K_MIN, CliqueEngine
from ..tc_engine import ORDERS
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    if a.order not in ORDERS:
        raise SystemExit(f"-order needs one of {', '.join(ORDERS)}")
    if not K_MIN <= a.clique <= K_MAX:
        raise SystemExit(f"-clique needs a size in {K_MIN}..{K_MAX}")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("clique is single-GPU for now: a row's bit matrix "
                         "needs its neighbours' rows on one device (run "
                         "with one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # oriented copy (<= one word per edge) + sort keys while it is built
    print_memory_estimate(part.nv, part.ne, 1, k=2)
    eng = CliqueEngine(part, k=a.clique, order=a.order)  # orient + items
    eng.timed = True
    with ElapsedTimer():
        total = eng.count()
    st, ph = eng.stats, eng.phase_ms
    print(f"[lux] clique: k {eng.k}, {total} cliques, "
          f"{st['simple_edges']} simple edges, max out-degree "
          f"{st['max_out_degree']}, spills {st['spills']}, phases "
          f"orient/items/count = "
          f"{ph['orient']:.3f}/{ph['items']:.3f}/{ph['count']:.3f} ms")
    if a.verbose:
        print("role,class,items")
        for name, _, cls, it in eng.items:
            print(f"{name.rstrip('0123456789')},{cls},{it.shape[0]}")
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
