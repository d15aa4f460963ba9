"""Collaborative filtering app driver (reference parity:
col_filter/colfilter.cc; SGD matrix-factorization sweeps, rank -k).
-als selects the exact ALS optimizer, -als -implicit [-alpha A] [-reg L] the
implicit-feedback ALS (CFImplicitALSEngine)."""
import sys

from .. import dist as dx
from ..cf_engine import CFALSEngine, CFEngine
from ..engine import GraphPart
from .common import (ElapsedTimer, load_part, parse_input_args,
                     print_memory_estimate)

# NetFlix-prize shape (reference README.md:86: 497,959 V / 200,961,014 E)
NETFLIX_USERS = 480189
NETFLIX_ITEMS = 17770


def build_cf_bench(args, device):
    from ..engine import DeviceCSC
    ne = args.edges if args.edges != (1 << 31) else 200961014
    if dx.world_size() > 1:  # rank-sliced build: graph/P per rank
        part = GraphPart.bipartite_sliced(NETFLIX_USERS, NETFLIX_ITEMS, ne,
                                          dx.world_size(), dx.rank(),
                                          seed=args.seed, device=device)
    else:
        full = DeviceCSC.bipartite(NETFLIX_USERS, NETFLIX_ITEMS, ne,
                                   seed=args.seed, device=device)
        part = GraphPart(full, 1, 0)
    cls = CFALSEngine if getattr(args, "als", False) else CFEngine
    return cls(part, K=64), part


def main(argv=None):
    a = parse_input_args(sys.argv[1:] if argv is None else argv)
    if a.implicit and not a.als:
        raise SystemExit("-implicit is an ALS variant: add -als")
    if a.implicit and not 1 <= a.k <= 64:
        raise SystemExit("-implicit covers -k 1..64")
    dx.init_process_group("cuda")
    import torch
    local = dx.env_local_rank()
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    part = load_part(a, device, weighted=True)
    if a.users and part.n_users is None:  # -file graphs don't carry the
        part.n_users = a.users            # boundary; -users supplies it
    if dx.rank() == 0:
        print_memory_estimate(part.nv, part.ne, dx.world_size(),
                              weighted=True, k=a.k)
    if a.implicit:
        from ..cf_ials_engine import CFImplicitALSEngine
        if part.n_users is None:
            raise SystemExit("-implicit needs the user/item boundary: "
                             "-users N or a bipartite spec")
        try:
            eng = CFImplicitALSEngine(part, K=a.k, alpha=a.alpha, reg=a.reg)
        except ValueError as e:
            raise SystemExit(f"-implicit: {e}")
    else:
        eng = (CFALSEngine if a.als else CFEngine)(part, K=a.k)
    with ElapsedTimer():
        for _ in range(a.num_iter):
            eng.step()
    if a.implicit and a.num_iter > 0 and dx.rank() == 0:
        ms = eng.phase_ms
        print("[lux] implicit ALS: alpha = %g, reg = %g; last sweep: side "
              "Gram %.3f ms, row solves %.3f ms, hub rows %.3f ms; %d hub "
              "rows, %d chunk slots, %d scratch bytes"
              % (a.alpha, a.reg, ms["side_gram"], ms["solve"], ms["hub"],
                 eng.stats["hub_rows"], eng.stats["chunk_slots"],
                 eng.stats["scratch_bytes"]))
    if a.topn:
        recommend(a, part, eng)
    return eng


def recommend(a, part, eng):
    """-topn N [-queries Q]: the N best unseen items of users 0..Q-1 from
    the trained factors, timed on its own."""
    import time

    import torch

    from ..cf_topn_engine import CFTopN
    if dx.world_size() > 1:
        raise SystemExit("-topn is single-rank")
    if part.n_users is None:
        raise SystemExit("-topn needs the user/item boundary: -users N or a "
                         "bipartite spec")
    nq = min(a.queries, part.n_users) if a.queries > 0 else part.n_users
    rec = CFTopN(part, eng.vectors())
    users = torch.arange(nq, dtype=torch.int32, device=part.col.device)
    rec.seen()  # the exclusion rows are built once, outside the timing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    items, scores = rec.recommend(users, n=a.topn)
    torch.cuda.synchronize()
    print("TOPN TIME = %7.7f s (%d users x %d items, n = %d, %d splits)"
          % (time.perf_counter() - t0, nq, part.nv - part.n_users, a.topn,
             rec.stats["splits"]))
    print(f"check() = {rec.check()}")
    for u in range(min(nq, 3)):
        row = ", ".join(f"{i}:{s:.4f}" for i, s in
                        zip(items[u].tolist(), scores[u].tolist()))
        print(f"user {u}: {row}")
    return rec


if __name__ == "__main__":
    main()
