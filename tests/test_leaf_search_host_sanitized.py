"""CPU: the native placement search's host state (csrc/nep_leaf_search.cpp: slots' move records, the neighbours' bytes,
counts and screens) under AddressSanitizer and UBSan, as a stand-alone program (tools/host_checks/leaf_search_main.cpp,
built with nep_leaf_repair.cpp, nep_leaf_moves.cpp and nep_leaf_swaps.cpp) run on the full move and swap lists of
tests/test_leaf_search_cpu.py's cases.  Nothing is loaded into Python and nothing touches a GPU."""
import os
import subprocess

import numpy as np
import pytest

import leaf_search_ref as qref
from leaf_moves_cases import NAMES as _ALL, case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "neptune-mip_amd", "csrc")
MAIN = os.path.join(REPO, "tools", "host_checks", "leaf_search_main.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = [name for name in _ALL if name != "wide"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("leaf_search_host") / "leaf_search_check")
    src = [MAIN] + [os.path.join(CSRC, s) for s in ("nep_leaf_search.cpp", "nep_leaf_repair.cpp", "nep_leaf_moves.cpp",
                                                    "nep_leaf_swaps.cpp")]
    # (the sanitizers instrument the host code only: the sources hold no device code, and none is to be instrumented)
    r = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-ffp-contract=off", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe] + src,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout
    return exe


def _write(path, inst, z, moves):
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, np.float64).ravel())
    with open(path, "w") as f:
        f.write(f"{inst.F} {inst.N} {1 if inst.has_n else 0} {float(inst.budget)!r}\n")
        f.write(num(inst.fmem) + "\n" + num(inst.nmem) + "\n" + num(inst.cost) + "\n" + num(z) + "\n")
        f.write(f"{len(moves)}\n")
        for kind, fn, node, src in moves:
            f.write(f"{kind} {fn} {node} {-1 if src is None else src}\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_state_under_sanitizers(program, tmp_path, name):
    g = case(name)
    inst = g.inst
    ks = range(len(g.Z)) if name.startswith("fixture") else [0]
    total = 0
    for k in ks:
        moves = qref.full_moves(inst, g.Z[k])
        # records out of range are refused, not applied
        moves = moves + [(4, 0, 0, None), (0, inst.F, 0, None), (1, 0, inst.N, None), (3, 0, 0, inst.N), (2, -1, -1, None)]
        path = str(tmp_path / f"{name}_{k}.txt")
        _write(path, inst, g.Z[k], moves)
        r = subprocess.run([program, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, (name, k, r.stdout[-4000:])
        assert r.stdout.startswith("ok "), r.stdout
        total += int(r.stdout.split()[1])
    print(name, "moves checked", total)
    assert total > 0
