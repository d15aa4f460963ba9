"""Personalised PageRank app driver (no reference equivalent): one random
walk with restart per source -start, -start + 1, ... (modulo nv; -nsrc K,
default 64), up to 64 columns per sweep. -ni N iterations (default 10),
-damping D (default 0.85), -tol T stops a batch at the first residual <= T,
-top M vertices are printed per source (default 5). -verbose adds the
residual CSV, -check runs the device oracle on the last iteration. Single
GPU."""
import sys

from .. import dist as dx
from ..ppr_engine import PPREngine
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse_input_args(argv)
    nsrc = a.nsrc if "-nsrc" in argv else 64
    if nsrc < 1:
        raise SystemExit("-nsrc K needs K >= 1")
    dx.init_process_group("cuda")
    if dx.world_size() > 1:
        raise SystemExit("ppr is single-GPU for now: a sweep gathers the "
                         "rows of every in-neighbour on one device (run "
                         "with one process)")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device)
    # two state buffers of up to 64 columns and the [nv, K] result
    print_memory_estimate(part.nv, part.ne, 1, k=min(nsrc, 64) + nsrc // 2)
    eng = PPREngine(part)  # preparation
    eng.timed = True
    sources = [(a.start + i) % part.nv for i in range(nsrc)]
    try:
        with ElapsedTimer():
            eng.run(sources, iters=a.num_iter, tol=a.tol, damping=a.damping)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    st, ph, its = eng.stats, eng.phase_ms, eng.iterations()
    per_it = ", ".join(f"{n} x {ms / n:.3f} ms"
                       for n, ms in zip(its, eng.batch_ms))
    print(f"[lux] ppr: {nsrc} sources in {len(its)} batches, width "
          f"{st['width']}, damping {a.damping}, iterations per batch "
          f"[{per_it}], launches {st['launches']}, host reads "
          f"{st['host_reads']}, hub rows {st['hub_rows']}, phases plan/run = "
          f"{ph['plan']:.3f}/{ph['run']:.3f} ms")
    if a.top > 0:
        values, vertices = (t.tolist() for t in eng.topk(a.top))
        for s, val, ver in zip(sources, values, vertices):
            print(f"[lux] source {s}: " + " ".join(
                f"{v}:{x:.9g}" for v, x in zip(ver, val)))
    if a.verbose:
        print("batch,iteration,residual")
        for b, trace in enumerate(eng.residual_trace):
            for i, r in enumerate(trace):
                print(f"{b},{i},{r:.9g}")
    if a.check:
        mistakes = eng.check()
        tag = "PASS" if mistakes == 0 else "FAIL"
        print(f"[{tag}] {mistakes} mistakes")
    return eng


if __name__ == "__main__":
    main()
