"""numpy mirror of the priced moves of a fixed placement (nep_leaf_moves: csrc/nep_leaf_moves.hip prices,
csrc/nep_leaf_moves.cpp composes; DESIGN.md §7 "Priced moves") on leaf_ref.Instance, fp64, the same rules in the same
order.

At prices y >= 0 a loaded row r = (f, i) costs rho_r(j) = (kobj w) D[i, j] + w (y_j cpr[f, j]) at j (leaf_ref.assign's
expression).  m1_r / j1_r: its minimum and argmin over the open destinations of f (ties to the lowest j); m2_r: the
minimum over the others (+inf: none).  table[f, j] is the routing part of the change of L(y) when (f, j) flips."""
import math

import numpy as np

import leaf_ref

ADD, DROP, CLOSE = 0, 1, 2


def price_table(inst, C, y, n=None):
    """(table [F, N], lagr) of the placement C (n: its open nodes; None: the nodes with a placement) at prices y; a
    rejected placement: a table of +inf, lagr +inf."""
    N, F = inst.N, inst.F
    if n is None and inst.has_n:
        n = (C.sum(axis=0) > 0.5).astype(np.float64)
    y = np.zeros(N) if y is None else np.asarray(y, np.float64)
    table = np.full((F, N), math.inf)
    if leaf_ref.rejects(inst, C, n):
        return table, math.inf
    sf = 0.0
    for f in range(F):
        is_open = C[f] > 0.5
        op = np.flatnonzero(is_open)
        r0, r1 = inst.frow[f], inst.frow[f + 1]
        src = inst.row_src[r0:r1]
        src = src[src >= 0]
        nl = len(src)
        table[f, ~is_open] = 0.0
        if op.size > 1:
            table[f, op] = 0.0
        if nl == 0:
            continue
        w = inst.W[f, src]
        oc = inst.kobj * w
        rho = oc[:, None] * inst.D[src, :] + w[:, None] * (y * inst.cpr[f])[None, :]      # [rows, N]
        ro = rho[:, op]
        k1 = np.argmin(ro, axis=1)
        m1 = ro[np.arange(nl), k1]
        if op.size > 1:
            rest = ro.copy()
            rest[np.arange(nl), k1] = math.inf
            m2 = rest.min(axis=1)
        else:
            m2 = np.full(nl, math.inf)
        for j in np.flatnonzero(~is_open):
            s = 0.0
            for d in (m1 - rho[:, j]).tolist():
                s += d if d > 0.0 else 0.0
            table[f, j] = 0.0 - s
        if op.size > 1:
            gap = m2 - m1
            for k, j in enumerate(op.tolist()):
                s = 0.0
                for q in range(nl):
                    s += gap[q] if k1[q] == k else 0.0
                table[f, j] = s
        # the function's part of L(y), in the kernel's order: 64 strided partials, then a butterfly
        part = np.zeros(64)
        for q in range(nl):
            part[q % 64] += m1[q]
        o = 32
        while o:
            part = part + part[np.arange(64) ^ o]
            o >>= 1
        sf += part[0]
    sy = 0.0
    for j in range(N):
        sy += y[j] * inst.cores[j]
    base = inst.cost_n * float(n.sum()) if n is not None else 0.0
    return table, base + sf - sy


def move_list(inst, C, n, table, max_moves, screened=None):
    """[(kind, fn, node, delta)] in ascending (delta, kind, node, fn) order, at most max_moves; `screened` (a list)
    collects the (f, j) whose ADD the memory or budget screen dropped."""
    N, F = inst.N, inst.F
    if leaf_ref.rejects(inst, C, n):
        return []
    cn = inst.cost_n if inst.has_n else 0.0
    out = []
    for j in range(N):
        mem, closing, cnt, finite = 0.0, 0.0, 0, True
        for f in range(F):
            if C[f, j] > 0.5:
                mem += inst.fmem[f]
                cnt += 1
                if math.isfinite(table[f, j]):
                    closing += table[f, j]
                else:
                    finite = False
        opens = cnt == 0
        for f in range(F):
            t = float(table[f, j])
            if not C[f, j] > 0.5:
                if not mem + inst.fmem[f] <= inst.nmem[j] + 1e-9 or \
                        (opens and inst.has_n and not inst.cost[j] <= inst.budget + 1e-9):
                    if screened is not None:
                        screened.append((f, j))
                    continue
                out.append((t + (cn if opens else 0.0), ADD, j, f))
            elif math.isfinite(t):
                out.append((t - (cn if cnt == 1 else 0.0), DROP, j, f))
        if cnt >= 2 and finite:
            out.append((closing - cn, CLOSE, j, -1))
    out.sort()
    return [(k, f, j, d) for d, k, j, f in out[:max(0, max_moves)]]


def apply_move(inst, z, kind, fn, node):
    """z' of the move, through the product's apply_move (core/engine/heuristics.py)"""
    from core.engine.heuristics import apply_move as product
    return product(z, inst.F, inst.N, inst.has_n, kind, fn, node)


def lagrangian(inst, z, y):
    """L(C, y) recomputed by leaf_ref.assign, summed as leaf_ref.bound_rounds does"""
    C, n = inst.split(z)
    _, fpart, _ = leaf_ref.assign(inst, C, np.asarray(y, np.float64))
    return (inst.cost_n * float(n.sum()) if n is not None else 0.0) + float(fpart.sum()) - float(y @ inst.cores)


class MirrorModel:
    """leaf_eval / leaf_moves / leaf_routing of LPModel over the mirrors, so core.engine.heuristics.placement_search
    runs on the CPU unchanged."""

    def __init__(self, inst):
        self.inst, self.F, self.N = inst, inst.F, inst.N
        self.n_int = inst.F * inst.N + (inst.N if inst.has_n else 0)
        self._last = []

    def leaf_eval(self, z, rounds=32, cutoff=math.inf, prices=None, tol=0.0, repair_every=None):
        z = np.asarray(z, np.float64).reshape(-1, self.n_int)
        if repair_every:
            import leaf_heur_ref
            res = [leaf_heur_ref.leaf_eval_ex(self.inst, zb, rounds=rounds, every=int(repair_every), cutoff=cutoff,
                                              prices=None if prices is None else np.asarray(prices)[b])
                   for b, zb in enumerate(z)]
        else:
            res = [leaf_ref.leaf_eval(self.inst, zb, rounds=rounds, cutoff=cutoff, tol=tol or 1e-6,
                                      prices=None if prices is None else np.asarray(prices)[b])
                   for b, zb in enumerate(z)]
        self._last = res
        return {"lower": np.array([r["lower"] for r in res]), "upper": np.array([r["upper"] for r in res]),
                "status": np.array([r["status"] for r in res], np.int32),
                "prices": np.array([r["prices"] for r in res]), "cpu": np.array([r["cpu"] for r in res])}

    def leaf_routing(self, k):
        return self._last[k]["entries"]

    def leaf_moves(self, z, prices=None, max_moves=64, table=False):
        z = np.asarray(z, np.float64).reshape(-1, self.n_int)
        n, mm = len(z), int(max_moves)
        out = {"n_moves": np.zeros(n, np.int32), "kind": np.full((n, mm), -1, np.int32),
               "fn": np.full((n, mm), -1, np.int32), "node": np.full((n, mm), -1, np.int32),
               "delta": np.full((n, mm), math.inf), "lagr": np.zeros(n)}
        tabs = []
        for b, zb in enumerate(z):
            C, nn = self.inst.split(zb)
            tab, out["lagr"][b] = price_table(self.inst, C, None if prices is None else np.asarray(prices)[b], nn)
            tabs.append(tab)
            mv = move_list(self.inst, C, nn, tab, mm)
            out["n_moves"][b] = len(mv)
            for q, (k, f, j, d) in enumerate(mv):
                out["kind"][b, q], out["fn"][b, q], out["node"][b, q], out["delta"][b, q] = k, f, j, d
        if table:
            out["table"] = np.array(tabs)
        return out
