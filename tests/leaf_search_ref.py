"""The mirror model of the native placement search's suites (tests/test_leaf_search_cpu.py): leaf_swaps_ref.MirrorModel
whose leaf_eval also returns device_upper — the device's own best objective per placement, from
leaf_heur_ref.leaf_eval_ex — which core.engine.heuristics.placement_search(verify="lazy") ranks its candidates by.
full_moves: every move and swap of a placement (zero prices: the lists' screens do not depend on the prices)."""
import numpy as np

import leaf_moves_ref
import leaf_swaps_ref


class MirrorModel(leaf_swaps_ref.MirrorModel):
    def leaf_eval(self, z, rounds=32, cutoff=np.inf, prices=None, tol=0.0, repair_every=None):
        out = super().leaf_eval(z, rounds=rounds, cutoff=cutoff, prices=prices, tol=tol, repair_every=repair_every)
        if repair_every:
            out["device_upper"] = np.array([r["device_upper"] for r in self._last], np.float64)
        return out


def full_moves(inst, z):
    """[(kind, fn, node, src or None)]: the whole move list and the whole swap list of the placement z at zero prices,
    in the lists' order ([] for a placement the evaluator rejects)"""
    C, n = inst.split(z)
    y = np.zeros(inst.N)
    table, _ = leaf_moves_ref.price_table(inst, C, y, n)
    moves = leaf_moves_ref.move_list(inst, C, n, table, 2 * inst.F * inst.N + inst.N)
    out = [(k, f, j, None) for k, f, j, _ in moves]
    if moves:
        best, best_from = leaf_swaps_ref.swap_tables(inst, C, y, n)
        out += [(3, f, to, src) for f, src, to, _ in leaf_swaps_ref.swap_list(best, best_from, inst.N, inst.F * inst.N)]
    return out
