"""Triangle counting app driver (no reference equivalent): exact count on
the underlying simple undirected graph of -file / -synthetic, oriented by
-order degree (default) or id. Single GPU."""
import sys

from .. import dist as dx
from ..tc_engine import ORDERS, ROLES, TCEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    if a.order not in ORDERS:
        raise SystemExit(f"-order needs one of {', '.join(ORDERS)}")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("tc is single-GPU for now: an intersection needs "
                         "both rows on one device (run with one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # oriented copy (<= one word per edge) + sort keys while it is built
    print_memory_estimate(part.nv, part.ne, 1, k=2)
    eng = TCEngine(part, order=a.order)  # preparation: orient + items
    eng.timed = True
    with ElapsedTimer():
        total = eng.count()
    st, ph = eng.stats, eng.phase_ms
    print(f"[lux] tc: {total} triangles, {st['simple_edges']} simple edges, "
          f"transitivity {eng.transitivity():.6f}, max out-degree "
          f"{st['max_out_degree']}, phases orient/items/count = "
          f"{ph['orient']:.3f}/{ph['items']:.3f}/{ph['count']:.3f} ms")
    if a.verbose:
        from ..trace import IterTrace
        tr = IterTrace()
        for role in ROLES:
            tr.record(role=role, items=st[f"items_{role}"])
        tr.record(role="all", items=sum(st[f"items_{r}"] for r in ROLES),
                  probes=st["probes"])
        print(tr.to_csv(), end="")
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
