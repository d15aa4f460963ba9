"""Betweenness centrality app driver (no reference equivalent): Brandes
dependency accumulation from -start, or summed over the -nsrc sources
-start, -start + 1, ... (modulo nv). Single GPU."""
import sys

from .. import dist as dx
from ..bc_engine import BCEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    if a.nsrc < 1:
        raise SystemExit("-nsrc N needs N >= 1")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("bc is single-GPU for now: the delta pass needs a "
                         "per-level sum across ranks (run with one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # 8-byte records + sigma, delta, bc + the two work lists: ~7 words/vertex
    print_memory_estimate(part.nv, part.ne, 1, k=4)
    eng = BCEngine(part)
    eng.timed = True
    sources = [(a.start + i) % part.nv for i in range(a.nsrc)]
    with ElapsedTimer():
        eng.run_sources(sources)
    reached = int((eng.depth() != -1).sum().item())
    ph = eng.phase_ms
    print(f"[lux] bc: {eng.levels} levels, {reached} reached, phases "
          f"bfs/order/sigma/delta = {ph['bfs']:.3f}/{ph['order']:.3f}/"
          f"{ph['sigma']:.3f}/{ph['delta']:.3f} ms")
    if a.verbose:
        from ..trace import IterTrace
        tr = IterTrace()
        for row in eng.stats:
            tr.record(**row)
        print(tr.to_csv(), end="")
    if a.check:
        # the oracle recomputes the last source's sigma and delta
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
