#!/usr/bin/env python3
"""Writes tests/golden/leaf_eval.json: fixed placements of small synthetic step-1 instances with the HiGHS value of
their leaf LP (oracle/) and what the numpy mirror of the fixed-placement evaluator (tests/leaf_ref.py) returns for them.
CPU only.  The placements are MIP optima (or a time-limited HiGHS incumbent) and those with their last open node
closed, which congests or breaks the routing.

    python tools/gen_leaf_golden.py
"""
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "neptune-mip_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from core.utils import data_to_solver_input            # noqa: E402
from core.utils.synthetic import synthetic_payload     # noqa: E402
from oracle.formulation import build_model             # noqa: E402
from oracle.inputs import data_to_solver_input as oracle_input   # noqa: E402
from oracle.solve import solve                         # noqa: E402
import leaf_ref                                        # noqa: E402

# (N, F, seed, rho, variant, MIP time limit or None, also with the last open node closed)
INSTANCES = [
    (16, 8, 0, 0.1, "MinDelayAndUtilization", None, False),
    (24, 12, 0, 0.1, "MinDelayAndUtilization", None, False),
    (12, 6, 1, 1.0, "MinDelayAndUtilization", None, True),
    (24, 12, 2, 0.5, "MinDelayAndUtilization", 30.0, True),
    (20, 10, 3, 0.5, "MinDelayAndUtilization", None, True),
    (10, 5, 0, 0.5, "MinDelayAndUtilization", None, True),       # (i) N not a multiple of 4
    (80, 2, 0, 0.5, "MinDelayAndUtilization", "wide", True),   # (ii) a function open at more than 64 destinations
    (16, 8, 0, 0.1, "MinDelay", None, False),                    # (iii)
    (16, 8, 0, 0.1, "MinUtilization", None, False),
    (16, 8, 0, 0.1, "MinDelayAndUtilization", "all-open", False),   # C3 rejects it: INFEASIBLE without a round
]


def close_last(z, N, F, has_n):
    z = z.copy()
    C = z[:F * N].reshape(F, N)
    j = int(np.flatnonzero(C.sum(axis=0) > 0.5)[-1])
    C[:, j] = 0.0
    if has_n:
        z[F * N + j] = 0.0
    return z


def main():
    cases = []
    for N, F, seed, rho, variant, limit, closed in INSTANCES:
        p = synthetic_payload(N, F, seed=seed, rho=rho)
        alpha = p["solver"]["args"]["alpha"]
        data = data_to_solver_input(p, with_db=False)
        inst = leaf_ref.Instance(data, variant, alpha)
        model = build_model(oracle_input(p, with_db=False), variant, step=1, alpha=alpha)
        nx, ni = N * N * F, F * N + (N if inst.has_n else 0)
        if limit == "wide":
            z0 = np.ones(ni)
            z0[:F * N].reshape(F, N)[:, 7::8] = 0.0
            z0[F * N + 7::8] = 0.0
            assert not leaf_ref.rejects(inst, *inst.split(z0)), "the wide placement must pass C3"
            kind = "every node but each eighth open"
        elif limit == "all-open":
            z0 = np.ones(ni)
            assert leaf_ref.rejects(inst, *inst.split(z0)), "the all-open placement must break a memory row"
            kind = "every placement open"
        else:
            st, obj, x = solve(model, relax=False, time_limit=limit)
            assert x is not None, (N, F, seed, rho, variant)
            z0 = np.rint(x[nx:nx + ni])
            kind = "MIP optimum" if limit is None else f"HiGHS {limit:g} s incumbent"
        for z, what in [(z0, kind)] + ([(close_last(z0, N, F, inst.has_n), kind + ", last open node closed")] if closed
                                       else []):
            lb, ub = model["lb"].copy(), model["ub"].copy()
            lb[nx:nx + ni] = ub[nx:nx + ni] = z
            st, lp, _ = solve(model, relax=True, lb=lb, ub=ub)
            r0 = leaf_ref.leaf_eval(inst, z, rounds=0)
            r64 = leaf_ref.leaf_eval(inst, z, rounds=64)
            # exact ties (equal integer delays, e.g. two nodes at rounded distance 0) are decided by the tie rule; a tie
            # that only rounding decides would make the fixture depend on the order of operations
            assert r64["ties"][1] == 0, f"the mirror's repair met a near tie: {(N, F, seed, rho, variant, what)}"
            C, n = inst.split(z)
            case = {"N": N, "F": F, "seed": seed, "rho": rho, "variant": variant, "alpha": alpha, "placement": what,
                    "c": C.astype(int).tolist(), "n": None if n is None else n.astype(int).tolist(),
                    "lp_status": int(st), "lp_value": lp,
                    "lower0": r0["lower"] if math.isfinite(r0["lower"]) else None,
                    "lower64": r64["lower"] if math.isfinite(r64["lower"]) else None,
                    "repair_exact_ties": int(r64["ties"][0]), "status0": int(r0["status"]), "status64": int(r64["status"]),
                    "upper": r64["upper"] if math.isfinite(r64["upper"]) else None}
            print({k: v for k, v in case.items() if k not in ("c", "n")}, flush=True)
            cases.append(case)
    out = os.path.join(REPO, "tests", "golden", "leaf_eval.json")
    with open(out, "w") as f:
        json.dump({"generator": "tools/gen_leaf_golden.py", "cases": cases}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
