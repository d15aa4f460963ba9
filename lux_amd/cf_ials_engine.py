"""Implicit-feedback ALS (Hu, Koren, Volinsky 2008) on the GPU, K <= 64
(src/gpu/cf_ials.hip; definition in API.md).

Every user/item pair enters the loss: unobserved pairs with confidence 1 and
preference 0, observed ones with confidence 1 + alpha * w and preference 1.
A phase therefore needs Y^T Y over the WHOLE opposite side (one tall-skinny
MFMA reduction per phase) before the per-row solves, which start their
accumulators from it. Same init, split bin lists, half-step protocol and
publish as CFALSEngine; every rank holds the whole factor table, so each
computes the opposite side's Gram itself (same kernel, same bits) and no new
communication is needed."""
import torch

from . import _native_gpu as ng
from . import dist as dx
from .cf_engine import als_init
from .engine import GraphPart

F32 = torch.float32
I32 = torch.int32
CHUNK_EDGES = 8192  # entries per hub chunk (pull.hip)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class CFImplicitALSEngine:
    def __init__(self, part: GraphPart, K=64, alpha=40.0, reg=0.01):
        if part.weight is None:
            raise ValueError("implicit ALS needs a weighted graph")
        if part.n_users is None:
            raise ValueError("implicit ALS needs the user/item boundary: "
                             "-users N or a bipartite spec")
        if not 1 <= K <= 64:
            raise ValueError(f"implicit ALS covers 1 <= K <= 64, got {K}")
        if not alpha > 0 or not reg > 0:
            raise ValueError(f"alpha and reg must be > 0, got alpha={alpha}, "
                             f"reg={reg}")
        if part.ep and int(part.weight[:part.ep].min()) < 0:
            raise ValueError("implicit ALS takes weights >= 0 (interaction "
                             "counts)")
        self.part = part
        self.K, self.alpha, self.reg = K, float(alpha), float(reg)
        part.build_bins()
        device = part.device
        self.old = torch.from_numpy(als_init(part.nv, K)).to(device)
        self.new_part = torch.empty(part.vp * K, dtype=F32, device=device)
        self.verts_elems = [v * K for v in part.verts_all]
        self.left_elems = [l * K for l in part.row_left_all]
        nu = part.n_users
        self.lb = lb = min(max(nu - part.row_left, 0), part.vp)

        # stable-partition the fused-row lists: local user rows first
        def _split(t, n):
            t = t[:n]
            m = t < lb
            return torch.cat([t[m], t[~m]]), int(m.sum())
        self.bin0s, self.n0u = _split(part.bin0, part.n0)
        self.bin1s, self.n1u = _split(part.bin1, part.n1)
        # Hub rows ascending (users first, as local ids are), their chunks in
        # (row, chunk) order: chunk entry i owns scratch slot i, so a hub's
        # partial sums are added in chunk order whatever order the bin
        # builder's atomics produced. Slots are phase-relative.
        hubs = part.bin2v[:part.nbig].long().sort().values
        self.nbigu = int((hubs < lb).sum())
        self.bin2vs = hubs.to(I32)
        rp = part.row_ptr.long()
        nch = (rp[hubs + 1] - rp[hubs] + CHUNK_EDGES - 1) // CHUNK_EDGES
        self.phase = {}
        for name, sl in (("users", slice(0, self.nbigu)),
                         ("items", slice(self.nbigu, part.nbig))):
            h, c = hubs[sl], nch[sl]
            first = torch.zeros(len(h) + 1, dtype=torch.int64, device=device)
            first[1:] = torch.cumsum(c, 0)
            n2 = int(first[-1])
            rows = torch.repeat_interleave(h, c)
            idx = torch.arange(n2, device=device) \
                - torch.repeat_interleave(first[:-1], c)
            self.phase[name] = dict(
                nbig=len(h), n2=n2, hubs=h.to(I32).contiguous(),
                first=first.to(I32),
                chunks=torch.stack([rows, idx], 1).to(I32).reshape(-1))
        slot_f = ng.cf_ials_slot_floats()
        self.slots_n = max(ph["n2"] for ph in self.phase.values())
        self.slots = torch.empty(self.slots_n * slot_f, dtype=F32,
                                 device=device) if self.slots_n else None
        gram_f = max(ng.cf_ials_gram_scratch_floats(nu),
                     ng.cf_ials_gram_scratch_floats(part.nv - nu))
        self.gram_scratch = torch.empty(max(gram_f, 1), dtype=F32,
                                        device=device)
        self.gram = torch.empty(64 * 64, dtype=F32, device=device)
        self.stats = {"launches": 0, "hub_rows": part.nbig,
                      "chunk_slots": self.slots_n,
                      "scratch_bytes": 4 * (self.slots_n * slot_f + gram_f)}
        self._ev, self._launches = {}, {}

    def _side_gram_into(self, side, out):
        nu, nv = self.part.n_users, self.part.nv
        lo, hi = (0, nu) if side == "users" else (nu, nv)
        return ng.cf_ials_side_gram(_stream(), self.old, lo, hi, self.K,
                                    self.gram_scratch, out)

    def side_gram(self, side):
        """Unregularised 64x64 Y^T Y of the CURRENT factors of one side
        ("users" | "items"); rows and columns >= K are zero."""
        assert side in ("users", "items")
        out = torch.empty(64 * 64, dtype=F32, device=self.old.device)
        self._side_gram_into(side, out)
        return out.view(64, 64)

    def _publish(self):
        p = self.part
        dx.all_gather_slices(self.old, self.new_part, self.verts_elems,
                             self.left_elems, my_index=p.p)

    def half_step(self, phase):
        """One alternation phase + its publish: 'users' solves the user rows
        against the item factors, 'items' the item rows against the
        (published) users. Rows of the solved side without entries become
        zero; the other side's rows keep their bits."""
        assert phase in ("users", "items")
        p, K, lb = self.part, self.K, self.lb
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        self.new_part.copy_(self.old.narrow(0, p.row_left * K, p.vp * K))
        if phase == "users":
            self.new_part[:lb * K].zero_()
        else:
            self.new_part[lb * K:].zero_()
        ev[0].record()
        n = self._side_gram_into("items" if phase == "users" else "users",
                                 self.gram)
        ev[1].record()
        ph = self.phase[phase]
        if phase == "users":
            b0, n0, b1, n1 = self.bin0s, self.n0u, self.bin1s, self.n1u
        else:
            b0, n0 = self.bin0s[self.n0u:], p.n0 - self.n0u
            b1, n1 = self.bin1s[self.n1u:], p.n1 - self.n1u
        tail = (p.row_ptr, p.col, p.weight, self.old, self.new_part, K,
                self.gram, self.alpha, self.reg)
        s = _stream()
        if ph["nbig"]:
            n += ng.cf_ials_phase(s, 0, None, 0, None, ph["n2"], ph["chunks"],
                                  ph["nbig"], ph["hubs"], ph["first"],
                                  self.slots, *tail)
        ev[2].record()
        if n0 or n1:
            n += ng.cf_ials_phase(s, n0, b0, n1, b1, 0, None, 0, None, None,
                                  None, *tail)
        ev[3].record()
        self._ev[phase] = ev
        self._launches[phase] = n
        self.stats["launches"] = sum(self._launches.values())  # last sweep
        self._publish()

    @property
    def phase_ms(self):
        """Device milliseconds of the last users + items phases: side Gram,
        fused row solves, hub chunks + hub solves (synchronises)."""
        torch.cuda.synchronize()
        out = {"side_gram": 0.0, "hub": 0.0, "solve": 0.0}
        for ev in self._ev.values():
            out["side_gram"] += ev[0].elapsed_time(ev[1])
            out["hub"] += ev[1].elapsed_time(ev[2])
            out["solve"] += ev[2].elapsed_time(ev[3])
        return out

    def step(self):
        self.half_step("users")
        self.half_step("items")

    def vectors(self):
        return self.old.view(self.part.nv, self.K)
