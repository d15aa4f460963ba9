"""Betweenness centrality app driver (no reference equivalent): Brandes
dependency accumulation from -start, or summed over the -nsrc sources
-start, -start + 1, ... (modulo nv). -batch B (16 | 32 | 64) sends the
sources through BatchedBCEngine, B per level sweep. Single GPU."""
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
    if a.batch:
        return _main_batched(a, part)
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


def _main_batched(a, part):
    from ..bc_batch_engine import BatchedBCEngine
    B = a.batch
    # dep u16 + val, delta, kept sigma f32 per column, the MS-BFS depth rows
    # (i32 per column) and its out-edge CSR; bc and the lists ride in k
    print_memory_estimate(
        part.nv, part.ne, 1, k=4,
        extra=((2 + 4 * 3) * B + 4 * B + 8) * part.nv + 4 * part.ne)
    eng = BatchedBCEngine(part, width=B)
    eng.timed = True
    sources = [(a.start + i) % part.nv for i in range(a.nsrc)]
    if len(set(sources)) != len(sources):
        raise SystemExit(f"-nsrc {a.nsrc} wraps around the {part.nv} "
                         f"vertices: -batch needs distinct sources")
    with ElapsedTimer():
        eng.run(sources, keep_sigma=a.check)
    reached = int((eng.depths() != -1).sum().item())
    ph = eng.phase_ms
    print(f"[lux] bc: batch {B}, {eng.levels} levels, {reached} reached "
          f"(last batch), phases bfs/order/sigma/delta/reduce = "
          f"{ph['bfs']:.3f}/{ph['order']:.3f}/{ph['sigma']:.3f}/"
          f"{ph['delta']:.3f}/{ph['reduce']:.3f} ms")
    if a.verbose:
        from ..trace import IterTrace
        tr = IterTrace()
        for row in eng.stats:
            tr.record(**row)
        print(tr.to_csv(), end="")
    if a.check:
        # the oracle recomputes the last batch's sigma and delta
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
