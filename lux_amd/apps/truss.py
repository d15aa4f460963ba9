"""k-truss decomposition app driver (no reference equivalent): the
trussness of every edge of the underlying simple undirected graph of -file /
-synthetic; -truss K also reports the size of the K-truss. Single GPU."""
import sys

from .. import dist as dx
from ..truss_engine import TrussEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("truss is single-GPU for now: an intersection needs "
                         "both rows on one device (run with one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # both directions of every edge with their edge ids, seven words of
    # per-edge state and the sort keys while the adjacency is built
    print_memory_estimate(part.nv, part.ne, 1, k=8)
    eng = TrussEngine(part)  # preparation: orient + adjacency
    eng.timed = True
    with ElapsedTimer():
        eng.decompose()
    st, ph = eng.stats, eng.phase_ms
    sizes = eng.truss_sizes()
    print(f"[lux] truss: kmax {eng.kmax()}, innermost truss "
          f"{int(sizes[-1].item()) if sizes.numel() else 0} edges, "
          f"{st['simple_edges']} simple edges, max degree "
          f"{st['max_degree']}, roles lane/wave/hub = {st['items_lane']}/"
          f"{st['items_wave']}/{st['items_hub']}, levels {st['levels']}, "
          f"rounds {st['rounds']} ({st['fused_rounds']} fused), scans "
          f"{st['scans']}, launches {st['launches']}, host reads "
          f"{st['host_reads']}, hub items {st['hub_items']}, phases "
          f"orient/adjacency/support/peel = {ph['orient']:.3f}/"
          f"{ph['adjacency']:.3f}/{ph['support']:.3f}/{ph['peel']:.3f} ms")
    if a.truss is not None:
        print(f"[lux] truss: the {a.truss}-truss has "
              f"{int(eng.truss(a.truss).sum().item())} edges on "
              f"{eng.truss_vertices(a.truss)} vertices")
    if a.verbose:
        from ..trace import IterTrace
        tr = IterTrace()
        for k, rounds, removed in eng.level_trace:
            tr.record(k=k, rounds=rounds, removed=removed)
        print(tr.to_csv(), end="")
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
