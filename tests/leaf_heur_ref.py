"""numpy mirror of the fixed-placement evaluator's per-round repair (nep_leaf_eval_ex: csrc/nep_leaf_heur.hip,
csrc/nep_leaf_repair.cpp; DESIGN.md §7 "Fixed-placement evaluator"), on top of tests/leaf_ref.py, which stays as it is.

The price rounds of `leaf_ref.bound_rounds` each end in a priced assignment that pushes load off congested nodes.
`leaf_eval_ex` repairs the assignment of every selected round (rounds k, 2k, ... and the last one), starting from the
round's own loads (the per-function shares summed in ascending f: `leaf_ref.assign`'s `load`), keeps the cheapest point
(strict improvement: the earliest round wins) and returns the cheaper of that point and the round-0 repair of
`leaf_ref.leaf_eval`.  The per-round repair carries the device kernel's two stops: at most DEV_MOVES moves per round,
and a node whose excess does not shrink ends the round's repair.
"""
import math

import numpy as np

import leaf_ref
from leaf_ref import CUTOFF, EXACT, FEASIBLE, INFEASIBLE, MARGIN, MARGIN_FLOOR, NO_POINT, STALL

DEV_MOVES = 4096          # csrc/nep_leaf.h kLeafDevMoves


def repair(inst, C, n, asg, load=None, max_moves=leaf_ref.MAX_MOVES, shrink_stop=False):
    """`leaf_ref.repair` from given CPU loads `load` [N] (None: the flat row-order sums of asg, as `leaf_ref.repair`),
    with a move cap and (shrink_stop, the device kernel's) the stop at a move that does not shrink its node's excess.
    Returns dict(found, obj, entries, cpu, ties, nears, moves)."""
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
        if load is None:
            cpu[j] += inst.W[f, i] * inst.cpr[f, j]
        col[f, j] += 1.0
        node_rows[j].append(r)
    if load is not None:
        cpu = np.asarray(load, np.float64).copy()
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
            if best is None or moves >= max_moves:
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
            before = cpu[j]
            cpu[j] -= t * relief
            cpu[jd] += t * ld
            col[f, j] -= t
            col[f, jd] += t
            room[f] -= max(0.0, floor - col[f, j]) + max(0.0, floor - col[f, jd]) - d0
            moves += 1
            if shrink_stop and not cpu[j] < before:
                ok = False
                break
        if not ok:
            break
    if ok:
        for f in range(F):
            r = inst.frow[f + 1] - 1
            defs = [max(0.0, floor - col[f, j]) for j in opens[f]]
            if inst.row_src[r] >= 0:
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
    return dict(found=ok, obj=obj, entries=(row, dst, val), cpu=cpu, ties=ties, nears=nears, moves=moves)


def repaired(rd, rounds, every):
    """round rd of 0 .. rounds is repaired at repair_every = every: rounds k, 2k, ... and the last one"""
    return every >= 1 and ((rd > 0 and rd % every == 0) or rd == rounds)


def rounds_with_repair(inst, C, n, rounds, every=1, cutoff=math.inf, prices=None, keep=False):
    """`leaf_ref.bound_rounds` with a repair of every selected round's assignment from the round's loads.  Returns
    (hist, ybest, asg0, last loads, cut, per-round list of None / the repair's dict (keep: with the round's asg and
    load; else without its entries),
    (best objective, its round, its asg, its load) or None)."""
    N = inst.N
    y = np.zeros(N) if prices is None else np.asarray(prices, np.float64).copy()
    base = inst.cost_n * float(n.sum()) if n is not None else 0.0
    best, ybest, lam, stall = -math.inf, y.copy(), 1.0, 0
    hist, asg0, load, cut = [], None, None, False
    per, sel = [None] * (rounds + 1), None
    for rd in range(rounds + 1):
        asg, fpart, load = leaf_ref.assign(inst, C, y)
        if rd == 0:
            asg0 = asg
        g = load - inst.cores
        g[(y == 0.0) & (g < 0.0)] = 0.0
        if repaired(rd, rounds, every):
            r = repair(inst, C, n, asg, load, DEV_MOVES, True)
            if r["found"] and (sel is None or r["obj"] < sel[0]):
                sel = (r["obj"], rd, asg.copy(), load.copy())
            if keep:
                r.update(asg=asg.copy(), load=load.copy())
            else:
                r = {k: v for k, v in r.items() if k != "entries"}
            per[rd] = r
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
    return np.asarray(hist), ybest, asg0, load, cut, per, sel


def leaf_eval_ex(inst, z, rounds=32, every=1, cutoff=math.inf, tol=1e-6, prices=None):
    """nep_leaf_eval_ex of one placement z: `leaf_ref.leaf_eval`'s dict plus upper_round (-1: no point), device_upper
    (the best per-round objective, inf: none) and rounds (the per-round repairs: None where the round was not
    repaired, else dict(found, obj, ties, nears, moves))."""
    C, n = inst.split(z)
    out = dict(lower=math.inf, upper=math.inf, status=INFEASIBLE, prices=np.zeros(inst.N), cpu=np.zeros(inst.N),
               entries=None, hist=None, ties=(0, 0), upper_round=-1, device_upper=math.inf,
               rounds=[None] * (rounds + 1))
    if leaf_ref.rejects(inst, C, n):
        return out
    hist, ybest, asg0, load, cut, per, sel = rounds_with_repair(inst, C, n, rounds, every, cutoff, prices)
    out.update(lower=float(hist[-1]), prices=ybest, cpu=load, hist=hist, rounds=per)
    if sel is not None:
        out["device_upper"] = sel[0]
    if cut:
        out["status"] = CUTOFF
        return out
    found, obj, ent, cpu, ties = leaf_ref.repair(inst, C, n, asg0)
    out["ties"] = ties
    rnd = 0 if found else -1
    if sel is not None:
        r = repair(inst, C, n, sel[2], sel[3])            # the host's verified repair of the selected round
        if r["found"] and (not found or r["obj"] < obj):
            found, obj, ent, cpu, rnd = True, r["obj"], r["entries"], r["cpu"], sel[1]
    out["upper_round"] = rnd
    if not found:
        out["status"] = NO_POINT
        return out
    lower = out["lower"]
    out.update(upper=obj, cpu=cpu, entries=ent,
               status=EXACT if obj - lower <= tol * max(1.0, abs(lower)) else FEASIBLE)
    return out
