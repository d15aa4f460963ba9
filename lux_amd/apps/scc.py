"""Strongly connected components app driver (no reference equivalent): the
SCC label (the largest vertex id of the component) of every vertex of the
directed graph of -file / -synthetic. Single GPU."""
import sys

from .. import dist as dx
from ..scc_engine import SCCEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("scc is single-GPU for now: a traversal follows "
                         "edges in both directions on one device (run with "
                         "one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # the out-edge CSR (one more word per edge) and ten words per vertex
    print_memory_estimate(part.nv, part.ne, 1, k=2)
    eng = SCCEngine(part)  # preparation: the out-edge CSR
    eng.timed = True
    with ElapsedTimer():
        eng.decompose()
    st, ph = eng.stats, eng.phase_ms
    sizes = eng.sizes()
    label, size = eng.largest()
    print(f"[lux] scc: {eng.num_components()} SCCs, largest {size} vertices "
          f"(label {label}), {int((sizes == 1).sum().item())} single-vertex "
          f"SCCs")
    print(f"[lux] scc: trim rounds {st['trim_rounds']} (trimmed "
          f"{st['trimmed']}), pivot {st['pivot']}, fwbw {st['fwbw']}, reach "
          f"rounds {st['reach_rounds']}, colour rounds "
          f"{st['colour_rounds']} (sweeps {st['colour_sweeps']}), launches "
          f"{st['launches']}, host reads {st['host_reads']}, fused steps "
          f"{st['fused_steps']}, hub items {st['hub_items']}, max in/out "
          f"degree {st['max_in_degree']}/{st['max_out_degree']}, phases "
          f"csr/trim/fwbw/colour = {ph['csr']:.3f}/{ph['trim']:.3f}/"
          f"{ph['fwbw']:.3f}/{ph['colour']:.3f} ms")
    if a.verbose:
        print("kind,round,removed")
        for kind, rnd, removed in eng.events:
            print(f"{kind},{rnd},{removed}")
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
