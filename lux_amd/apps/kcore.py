"""k-core decomposition app driver (no reference equivalent): the coreness
of every vertex of the underlying simple undirected graph of -file /
-synthetic; -kcore K also reports the size of the K-core. Single GPU."""
import sys

from .. import dist as dx
from ..kcore_engine import KCoreEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("kcore is single-GPU for now: a peel round "
                         "decrements neighbours on one device (run with one "
                         "process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # oriented copy + both directions of it (<= three words per edge) and
    # the sort keys while the first is built
    print_memory_estimate(part.nv, part.ne, 1, k=4)
    eng = KCoreEngine(part)  # preparation: orient + adjacency
    eng.timed = True
    with ElapsedTimer():
        eng.decompose()
    st, ph = eng.stats, eng.phase_ms
    shells = eng.shell_sizes()
    print(f"[lux] kcore: degeneracy {eng.degeneracy()}, innermost core "
          f"{int(shells[-1].item()) if shells.numel() else 0} vertices, "
          f"{st['simple_edges']} simple edges, max degree "
          f"{st['max_degree']}, levels {st['levels']}, rounds "
          f"{st['rounds']} ({st['fused_rounds']} fused), scans "
          f"{st['scans']}, host reads {st['host_reads']}, phases "
          f"orient/adjacency/peel = {ph['orient']:.3f}/"
          f"{ph['adjacency']:.3f}/{ph['peel']:.3f} ms")
    if a.kcore is not None:
        print(f"[lux] kcore: the {a.kcore}-core has "
              f"{int(eng.core(a.kcore).sum().item())} vertices")
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
