"""numpy mirror of the priced swaps of a fixed placement (nep_leaf_swaps: csrc/nep_leaf_swaps.hip prices and selects,
csrc/nep_leaf_swaps.cpp merges; DESIGN.md §7 "Priced swaps") on leaf_ref.Instance, fp64, the same rules in the same
order.

SWAP (f, j -> j') moves function f from an open destination j to a closed one j'.  With rho_r, m1_r, k1_r (the place of
the minimum in the ascending open list oj) and m2_r as in leaf_moves_ref, and bucket k the loaded rows of f with
k1_r = k in ascending row order:

  A_k(j') = sum_{r in bucket k} (min(m1_r, rho_r(j')) - m1_r)
  S_k(j') = sum_{r in bucket k} (min(m2_r, rho_r(j')) - m1_r)
  A_tot   = sum_k A_k, ascending k
  g_k     = (S_k - A_k) - cost_n [node oj[k] holds only this placement]
  delta(f, oj[k], j') = (A_tot + g_k) + cost_n [node j' holds none]

j' is admissible under leaf_moves_ref.move_list's ADD screens; best[f, j'] is the smallest delta over k (ties to the
lowest k), best_from[f, j'] its oj[k]."""
import math

import numpy as np

import leaf_moves_ref
import leaf_ref

SWAP = 3


def _rows(inst, C, y, f):
    """(open list, sources, workloads, m1, k1, m2) of function f"""
    op = np.flatnonzero(C[f] > 0.5)
    src = inst.row_src[inst.frow[f]:inst.frow[f + 1]]
    src = src[src >= 0]
    nl = len(src)
    w = inst.W[f, src]
    if nl == 0 or op.size == 0:
        return op, src, w, np.zeros(0), np.zeros(0, np.int64), np.zeros(0)
    oc = inst.kobj * w
    ro = oc[:, None] * inst.D[src][:, op] + w[:, None] * (y[op] * inst.cpr[f, op])[None, :]
    k1 = np.argmin(ro, axis=1)
    m1 = ro[np.arange(nl), k1]
    if op.size > 1:
        rest = ro.copy()
        rest[np.arange(nl), k1] = math.inf
        m2 = rest.min(axis=1)
    else:
        m2 = np.full(nl, math.inf)
    return op, src, w, m1, k1, m2


def _node_state(inst, C):
    """(placements per node, memory used per node summed over its functions in ascending order)"""
    cnt = np.zeros(inst.N, np.int64)
    mem = np.zeros(inst.N)
    for f in range(inst.F):
        on = C[f] > 0.5
        mem[on] += inst.fmem[f]
        cnt[on] += 1
    return cnt, mem


def admissible(inst, cnt, mem, f, jp):
    """the ADD screens of leaf_moves_ref.move_list for (f, jp)"""
    if not mem[jp] + inst.fmem[f] <= inst.nmem[jp] + 1e-9:
        return False
    return not (cnt[jp] == 0 and inst.has_n and not inst.cost[jp] <= inst.budget + 1e-9)


def _parts(inst, y, f, rows, jp):
    """(A_tot, [S_k - A_k per k]) of function f at the closed destination jp"""
    op, src, w, m1, k1, m2 = rows
    K = op.size
    rho = (inst.kobj * w) * inst.D[src, jp] + w * (y[jp] * inst.cpr[f, jp])
    da = (np.minimum(rho, m1) - m1).tolist()
    ds = (np.minimum(rho, m2) - m1).tolist()
    ak, sk = [0.0] * K, [0.0] * K
    for r, k in enumerate(k1.tolist()):            # ascending rows: each bucket in ascending row order
        ak[k] += da[r]
        sk[k] += ds[r]
    atot = 0.0
    for k in range(K):
        atot += ak[k]
    return atot, [sk[k] - ak[k] for k in range(K)]


def swap_tables(inst, C, y, n=None):
    """(best [F, N], best_from [F, N] int32) of the placement C at prices y; a rejected placement: +inf and -1"""
    N, F = inst.N, inst.F
    if n is None and inst.has_n:
        n = (C.sum(axis=0) > 0.5).astype(np.float64)
    y = np.zeros(N) if y is None else np.asarray(y, np.float64)
    best = np.full((F, N), math.inf)
    best_from = np.full((F, N), -1, np.int32)
    if leaf_ref.rejects(inst, C, n):
        return best, best_from
    cn = inst.cost_n if inst.has_n else 0.0
    cnt, mem = _node_state(inst, C)
    for f in range(F):
        rows = _rows(inst, C, y, f)
        op = rows[0]
        for jp in np.flatnonzero(~(C[f] > 0.5)).tolist():
            if not admissible(inst, cnt, mem, f, jp):
                continue
            atot, gaps = _parts(inst, y, f, rows, jp)
            g, kb = math.inf, -1
            for k in range(op.size):
                gk = gaps[k] - (cn if cnt[op[k]] == 1 else 0.0)
                if gk < g:
                    g, kb = gk, k
            best[f, jp] = (atot + g) + (cn if cnt[jp] == 0 else 0.0)
            best_from[f, jp] = op[kb]
    return best, best_from


def swap_delta(inst, C, y, n, f, j, jp):
    """delta of SWAP (f, j -> jp): j open for f, jp closed for f; +inf when jp is screened"""
    y = np.zeros(inst.N) if y is None else np.asarray(y, np.float64)
    assert C[f, j] > 0.5 and not C[f, jp] > 0.5
    cn = inst.cost_n if inst.has_n else 0.0
    cnt, mem = _node_state(inst, C)
    if not admissible(inst, cnt, mem, f, jp):
        return math.inf
    rows = _rows(inst, C, y, f)
    k = int(np.flatnonzero(rows[0] == j)[0])
    atot, gaps = _parts(inst, y, f, rows, jp)
    return (atot + (gaps[k] - (cn if cnt[j] == 1 else 0.0))) + (cn if cnt[jp] == 0 else 0.0)


def swap_list(best, best_from, per_fn, max_moves):
    """[(fn, from, to, delta)]: per function the per_fn cheapest finite (delta, to), merged in ascending (delta, fn, to,
    from) order, at most max_moves"""
    out = []
    for f in range(best.shape[0]):
        kept = sorted((float(best[f, j]), j) for j in np.flatnonzero(np.isfinite(best[f])).tolist())[:per_fn]
        out += [(d, f, j, int(best_from[f, j])) for d, j in kept]
    out.sort()
    return [(f, src, j, d) for d, f, j, src in out[:max(0, max_moves)]]


def apply_swap(inst, z, fn, src, to):
    """z' of the swap, through the product's apply_move (core/engine/heuristics.py)"""
    from core.engine.heuristics import apply_move as product
    return product(z, inst.F, inst.N, inst.has_n, SWAP, fn, to, src)


class MirrorModel(leaf_moves_ref.MirrorModel):
    """leaf_moves_ref.MirrorModel with LPModel's leaf_swaps over the mirror"""

    def leaf_swaps(self, z, prices=None, per_fn=4, max_moves=64, table=False):
        z = np.asarray(z, np.float64).reshape(-1, self.n_int)
        n, mm = len(z), int(max_moves)
        out = {"n_moves": np.zeros(n, np.int32), "fn": np.full((n, mm), -1, np.int32),
               "from": np.full((n, mm), -1, np.int32), "to": np.full((n, mm), -1, np.int32),
               "delta": np.full((n, mm), math.inf), "lagr": np.zeros(n)}
        tabs = []
        for b, zb in enumerate(z):
            C, nn = self.inst.split(zb)
            y = None if prices is None else np.asarray(prices)[b]
            _, out["lagr"][b] = leaf_moves_ref.price_table(self.inst, C, y, nn)
            tabs.append(swap_tables(self.inst, C, y, nn))
            sw = swap_list(*tabs[-1], int(per_fn), mm)
            out["n_moves"][b] = len(sw)
            for q, (f, src, j, d) in enumerate(sw):
                out["fn"][b, q], out["from"][b, q], out["to"][b, q], out["delta"][b, q] = f, src, j, d
        if table:
            out["best"] = np.array([t[0] for t in tabs])
            out["best_from"] = np.array([t[1] for t in tabs])
        return out
