"""Multi-source BFS app driver (no reference equivalent): hop distances from
the -nsrc sources -start, -start + 1, ... (modulo nv; default 64), 64 per
machine word, and the closeness, harmonic and eccentricity figures summed
from them. -check keeps the depth matrix for the device oracle. Single
GPU."""
import sys

from .. import dist as dx
from ..msbfs_engine import MSBFSEngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse_input_args(argv)
    nsrc = a.nsrc if "-nsrc" in argv else 64
    if nsrc < 1:
        raise SystemExit("-nsrc N needs N >= 1")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("msbfs is single-GPU for now: a level reads the "
                         "words of every neighbour on one device (run with "
                         "one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    if nsrc > part.nv:
        raise SystemExit(f"-nsrc {nsrc} exceeds the {part.nv} vertices: the "
                         f"sources must be distinct")
    # the out-edge CSR (one word per edge), three u64 words, two u64 sums,
    # reach, two queues and the role lists: ~14 words per vertex
    print_memory_estimate(part.nv, 2 * part.ne, 1, k=7)
    if a.check:
        print(f"[lux] -check keeps the depth matrix: "
              f"{4 * nsrc * part.nv} bytes")
    eng = MSBFSEngine(part)  # preparation
    eng.timed = True
    sources = [(a.start + i) % part.nv for i in range(nsrc)]
    with ElapsedTimer():
        eng.run(sources, depths=a.check)
    st, ph = eng.stats, eng.phase_ms
    close = eng.closeness()
    best = int(close.argmax())
    top = int(eng.harmonic().argmax().item())
    print(f"[lux] msbfs: {nsrc} sources in {eng.seen().shape[0]} batches, "
          f"levels {st['levels']} (push {st['push_levels']} / pull "
          f"{st['pull_levels']}), launches {st['launches']}, host reads "
          f"{st['host_reads']}, pairs reached {int(eng.reached().sum())}, "
          f"edges scanned {st['edges_scanned']} of {nsrc * part.ne} "
          f"({st['edges_scanned'] / max(nsrc * part.ne, 1):.4f}), largest "
          f"eccentricity {int(eng.eccentricity().max())}, highest closeness "
          f"source {sources[best]} ({close[best]:.6f}), highest harmonic "
          f"vertex {top} ({float(eng.harmonic()[top].item()):.6f}), hub "
          f"rows in/out {st['hub_rows_in']}/{st['hub_rows_out']}, phases "
          f"csr/plan/run = {ph['csr']:.3f}/{ph['plan']:.3f}/"
          f"{ph['run']:.3f} ms")
    if a.verbose:
        print("batch,level,direction,frontier,volume,new_pairs")
        for row in eng.level_trace:
            print("%d,%d,%s,%d,%d,%d" % row)
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
