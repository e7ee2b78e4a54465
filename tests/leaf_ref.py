"""numpy mirror of the fixed-placement evaluator (nep_leaf_eval: csrc/nep_leaf.hip, csrc/nep_leaf_repair.cpp;
DESIGN.md §7 "Fixed-placement evaluator"), fp64 throughout, the same rules in the same order.

A leaf fixes every c and n of a step-1 reference model.  What is left is one routing simplex per row (C4), the N CPU
rows (C5) and the column floors (C2).  Pricing C5 with y >= 0 and dropping C2 gives

    L(y) = cost_n sum n + sum_{loaded rows r} min_{j open for f} (oc_r D[src_r, j] + w_r (y_j cpr[f, j])) - sum_j y_j cores_j

(oc_r = kobj W[f, src], w_r = W[f, src]; pooled zero-workload rows have neither cost nor CPU), a lower bound on the
leaf LP at every y >= 0.  `leaf_eval` runs `rounds` subgradient steps on y and repairs the round-0 assignment into a
routing that meets every row (`repair`).
"""
import math

import numpy as np

EXACT, FEASIBLE, NO_POINT, INFEASIBLE, CUTOFF = 0, 1, 2, 3, 4
# the step rule's constants (csrc/nep_leaf.hip kLeaf*): Polyak step theta = lam (target - L) / |g|^2 toward the cutoff
# when finite, else toward best + MARGIN max(|best - base|, FLOOR max(1, |best|)) — base = cost_n sum n is constant at
# a leaf, so the margin scales with the routing part of the bound; lam starts at 1 and halves after STALL rounds in a
# row that did not raise the best bound
MARGIN, MARGIN_FLOOR, STALL = 0.05, 1e-3, 4
MAX_MOVES = 100000


class Instance:
    """The evaluator's view of a step-1 instance: fp64 D / W / cpr, the aggregated routing rows of the engine
    (per function its loaded sources in ascending order, then one pooled row for its zero-workload sources) and the
    objective's coefficients in reference units (objectives.py:4-53)."""

    def __init__(self, data, variant, alpha=0.5):
        f64 = lambda a: np.ascontiguousarray(np.asarray(a, np.float64))
        self.N, self.F = N, F = len(data.nodes), len(data.functions)
        self.D = f64(data.node_delay_matrix).reshape(N, N)
        self.W = f64(data.workload_matrix).reshape(F, N)
        self.cpr = f64(data.core_per_req_matrix).reshape(F, N)
        self.cores = f64(data.node_cores_matrix).reshape(N)
        self.fmem = f64(data.function_memory_matrix).reshape(F)
        self.nmem = f64(data.node_memory_matrix).reshape(N)
        self.cost = f64(data.node_costs).reshape(N)
        self.budget = float(data.node_budget)
        self.maxd = f64(data.max_delay_matrix).reshape(F)
        self.variant = variant
        self.has_n = variant != "MinDelay"
        self.eps = 1e-6
        sumw = float(self.W.sum())
        self.kobj, self.cost_n = 0.0, 0.0
        if variant == "MinDelay":
            self.kobj = 1.0
        elif variant == "MinDelayAndUtilization":
            self.cost_n = alpha / N
            if sumw != 0.0:
                mwd = 0.0
                for f in range(F):
                    for i in range(N):
                        mwd += self.W[f, i] * self.D[i][self.D[i] <= self.maxd[f]].max()
                self.kobj = (1.0 - alpha) / mwd
        else:
            self.cost_n = 1.0
        self.row_f, self.row_src, self.frow, self.m_f = [], [], [0], np.zeros(F)
        for f in range(F):
            src = np.flatnonzero(self.W[f] != 0.0)
            self.row_f += [f] * len(src)
            self.row_src += src.tolist()
            self.m_f[f] = N - len(src)
            if len(src) < N:
                self.row_f.append(f)
                self.row_src.append(-1)
            self.frow.append(len(self.row_f))
        self.row_f = np.asarray(self.row_f, np.int32)
        self.row_src = np.asarray(self.row_src, np.int32)
        self.R = len(self.row_f)

    def split(self, z):
        """(C [F, N], n [N] or None) of an integer vector z (c f-major, then n)."""
        z = np.asarray(z, np.float64)
        C = z[:self.F * self.N].reshape(self.F, self.N)
        return C, (z[self.F * self.N:self.F * self.N + self.N] if self.has_n else None)


def rejects(inst, C, n):
    """A row without x rejects the placement: C3 memory, C6/C7 n against c, C8 budget, or a function with no open
    destination (its C4 rows cannot hold under C1)."""
    if ((inst.fmem @ C) > inst.nmem + 1e-9).any():
        return True
    if (C.sum(axis=1) < 0.5).any():
        return True
    if n is not None:
        if ((C.sum(axis=0) > 0.5) != (n > 0.5)).any():
            return True
        if (inst.cost * n > inst.budget + 1e-9).any():
            return True
    return False


def assign(inst, C, y):
    """One priced assignment: (asg [R] destination per row, -1 for pooled rows; fpart [F] the functions' summed
    row minima; load [N] CPU load by node).  Argmin ties go to the lowest j."""
    N, F = inst.N, inst.F
    asg = np.full(inst.R, -1, np.int32)
    fpart = np.zeros(F)
    load = np.zeros(N)
    for f in range(F):
        op = np.flatnonzero(C[f] > 0.5)
        r0, r1 = inst.frow[f], inst.frow[f + 1]
        src = inst.row_src[r0:r1]
        nl = int((src >= 0).sum())
        if nl == 0 or op.size == 0:
            continue
        src = src[:nl]
        w = inst.W[f, src]
        yc = y[op] * inst.cpr[f, op]
        cost = (inst.kobj * w)[:, None] * inst.D[np.ix_(src, op)] + w[:, None] * yc[None, :]
        k = np.argmin(cost, axis=1)
        asg[r0:r0 + nl] = op[k]
        s = 0.0
        for v in cost[np.arange(nl), k]:
            s += v
        fpart[f] = s
        share = np.zeros(op.size)
        for q in range(nl):
            share[k[q]] += w[q]
        load[op] += share * inst.cpr[f, op]      # (ascending f: the per-node pass's order)
    return asg, fpart, load


def bound_rounds(inst, C, n, rounds, cutoff=math.inf, prices=None):
    """The price rounds: returns (best L per round [rounds + 1, padded with the last value once stopped], the best
    prices, round-0 assignment, last loads, cut off)."""
    N = inst.N
    y = np.zeros(N) if prices is None else np.asarray(prices, np.float64).copy()
    base = inst.cost_n * float(n.sum()) if n is not None else 0.0
    best, ybest, lam, stall = -math.inf, y.copy(), 1.0, 0
    hist, asg0, load, cut = [], None, None, False
    for rd in range(rounds + 1):
        asg, fpart, load = assign(inst, C, y)
        if rd == 0:
            asg0 = asg
        g = load - inst.cores
        g[(y == 0.0) & (g < 0.0)] = 0.0
        sf = 0.0
        for v in fpart:
            sf += v
        sy = 0.0
        for j in range(N):
            sy += y[j] * inst.cores[j]
        L = base + sf - sy
        if L > best:
            best, ybest, stall = L, y.copy(), 0
        else:
            stall += 1
            if stall >= STALL:
                lam, stall = 0.5 * lam, 0
        hist.append(best)
        if best >= cutoff:
            cut = True
            break
        gg = float(g @ g)
        if gg == 0.0:
            break
        target = cutoff if math.isfinite(cutoff) else \
            best + MARGIN * max(abs(best - base), MARGIN_FLOOR * max(1.0, abs(best)))
        theta = lam * (target - L) / gg
        y = np.maximum(0.0, y + theta * g)
    hist += [hist[-1]] * (rounds + 1 - len(hist))
    return np.asarray(hist), ybest, asg0, load, cut


def repair(inst, C, n, asg):
    """The host repair (csrc/nep_leaf_repair.cpp): from the assignment asg, move overflow off overloaded nodes (ascending
    j; per move the least objective increase per unit of CPU relief, ties by lowest row then lowest destination; rows
    split), place the pooled rows on the column deficits, verify every row.  Returns (found, objective, (row, dst, val),
    cpu [N], (ties, near)) — ties counts moves whose best score another candidate shared exactly (decided by the
    tie rule, the same in both implementations), near those with another candidate within 1e-12 relative of it but not
    equal (decided by rounding: the fixture generator asserts there are none)."""
    N, F = inst.N, inst.F
    floor = 1.0 - inst.eps
    lim = inst.cores - 1e-12 * np.maximum(1.0, np.abs(inst.cores))
    ent = [dict() for _ in range(inst.R)]
    cpu = np.zeros(N)
    col = np.zeros((F, N))
    node_rows = [[] for _ in range(N)]
    opens = [np.flatnonzero(C[f] > 0.5).tolist() for f in range(F)]
    for r in range(inst.R):
        f, i = int(inst.row_f[r]), int(inst.row_src[r])
        if i < 0:
            continue
        j = int(asg[r])
        ent[r][j] = 1.0
        cpu[j] += inst.W[f, i] * inst.cpr[f, j]
        col[f, j] += 1.0
        node_rows[j].append(r)
    room = np.array([inst.m_f[f] - sum(max(0.0, floor - col[f, j]) for j in opens[f]) for f in range(F)])
    ok, moves, ties, nears = True, 0, 0, 0
    for j in range(N):
        if not cpu[j] > inst.cores[j]:
            continue
        while cpu[j] > lim[j]:
            best = None
            tie = near = False
            for r in node_rows[j]:
                v = ent[r].get(j, 0.0)
                if v <= 0.0:
                    continue
                f, i = int(inst.row_f[r]), int(inst.row_src[r])
                w = inst.W[f, i]
                relief = w * inst.cpr[f, j]
                if not relief > 0.0:
                    continue
                tsrc = min(v, max(0.0, col[f, j] - floor) + max(0.0, room[f]))
                need = (cpu[j] - lim[j]) / relief
                oc = inst.kobj * w
                for jd in opens[f]:
                    if jd == j:
                        continue
                    ld = w * inst.cpr[f, jd]
                    t = min(tsrc, need)
                    if ld > 0.0:
                        rm = lim[jd] - cpu[jd]
                        if not rm > 0.0:
                            continue
                        t = min(t, rm / ld)
                    if not t > 1e-15:
                        continue
                    key = (oc * (inst.D[i, jd] - inst.D[i, j]) / relief, r, jd)
                    if best is not None and key[0] != best[0][0] and \
                            abs(key[0] - best[0][0]) <= 1e-12 * max(1.0, abs(best[0][0])):
                        near = True
                    elif best is None or key[0] < best[0][0]:
                        near = False
                    if best is None or key[0] < best[0][0]:
                        best, tie = (key, t, ld, relief, f), False
                    elif key[0] == best[0][0]:
                        tie = True
                        if key < best[0]:
                            best = (key, t, ld, relief, f)
            if best is None or moves >= MAX_MOVES:
                ok = False
                break
            (_, r, jd), t, ld, relief, f = best
            ties += int(tie)
            nears += int(near)
            d0 = max(0.0, floor - col[f, j]) + max(0.0, floor - col[f, jd])
            v = ent[r][j]
            if t >= v:
                del ent[r][j]
            else:
                ent[r][j] = v - t
            if jd not in ent[r]:
                node_rows[jd].append(r)
            ent[r][jd] = ent[r].get(jd, 0.0) + t
            cpu[j] -= t * relief
            cpu[jd] += t * ld
            col[f, j] -= t
            col[f, jd] += t
            room[f] -= max(0.0, floor - col[f, j]) + max(0.0, floor - col[f, jd]) - d0
            moves += 1
        if not ok:
            break
    # the pooled rows pay the column deficits; the rest of their mass goes to the function's lowest open node
    if ok:
        for f in range(F):
            r = inst.frow[f + 1] - 1
            defs = [max(0.0, floor - col[f, j]) for j in opens[f]]
            if inst.row_src[r] >= 0:             # no pooled row: the loaded flow alone must meet the floors
                if max(defs) > 1e-12:
                    ok = False
                continue
            m, rest = inst.m_f[f], 1.0
            for j, d in zip(opens[f][1:], defs[1:]):
                if d > 0.0:
                    ent[r][j] = d / m
                    rest -= d / m
            if rest * m < defs[0]:
                ok = False
            else:
                ent[r][opens[f][0]] = rest
    # the point in output order (row-major, ascending destination), its CPU loads and objective, verified in fp64
    row, dst, val = [], [], []
    for r in range(inst.R):
        for j in sorted(ent[r]):
            if ent[r][j] > 0.0:
                row.append(r)
                dst.append(j)
                val.append(ent[r][j])
    row, dst, val = np.asarray(row, np.int32), np.asarray(dst, np.int32), np.asarray(val, np.float64)
    cpu = np.zeros(N)
    obj = inst.cost_n * float(n.sum()) if n is not None else 0.0
    rsum = np.zeros(inst.R)
    colt = np.zeros((F, N))
    for r, j, v in zip(row.tolist(), dst.tolist(), val.tolist()):
        f, i = int(inst.row_f[r]), int(inst.row_src[r])
        rsum[r] += v
        if i >= 0:
            cpu[j] += v * (inst.W[f, i] * inst.cpr[f, j])
            obj += (inst.kobj * inst.W[f, i]) * inst.D[i, j] * v
            colt[f, j] += v
        else:
            colt[f, j] += v * inst.m_f[f]
    if ok:
        ok = bool((cpu <= inst.cores).all() and (np.abs(rsum - 1.0) <= 1e-12).all() and
                  (colt >= (C > 0.5) * floor - 1e-12).all() and not (colt[C < 0.5] > 0.0).any())
    return ok, obj, (row, dst, val), cpu, (ties, nears)


def leaf_eval(inst, z, rounds=32, cutoff=math.inf, tol=1e-6, prices=None):
    """nep_leaf_eval of one placement z: dict(lower, upper, status, prices, cpu, entries, hist, ties)."""
    C, n = inst.split(z)
    out = dict(lower=math.inf, upper=math.inf, status=INFEASIBLE, prices=np.zeros(inst.N), cpu=np.zeros(inst.N),
               entries=None, hist=None, ties=(0, 0))
    if rejects(inst, C, n):
        return out
    hist, ybest, asg0, load, cut = bound_rounds(inst, C, n, rounds, cutoff, prices)
    out.update(lower=float(hist[-1]), prices=ybest, cpu=load, hist=hist)
    if cut:
        out["status"] = CUTOFF
        return out
    found, obj, ent, cpu, ties = repair(inst, C, n, asg0)
    out["ties"] = ties
    if not found:
        out["status"] = NO_POINT
        return out
    lower = out["lower"]
    out.update(upper=obj, cpu=cpu, entries=ent,
               status=EXACT if obj - lower <= tol * max(1.0, abs(lower)) else FEASIBLE)
    return out


def dense_x(inst, entries):
    """x[f, i, j] of a routing's entries (the pooled rows expanded over their sources): check_placement's input."""
    x = np.zeros((inst.F, inst.N, inst.N))
    for r, j, v in zip(*entries):
        f, i = int(inst.row_f[r]), int(inst.row_src[r])
        if i >= 0:
            x[f, i, j] = v
        else:
            x[f, inst.W[f] == 0.0, j] = v
    return x
