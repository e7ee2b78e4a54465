"""Resources of the native search's kernels (CPU: hipcc cross-compiles gfx950 with the compiler's resource remarks), in
the manner of tests/test_leaf_swaps_kernel_resources.py: leaf_search_expand, leaf_node_state and leaf_search_adopt copy
and count — none uses scratch or spills a register, and each stays at 8 waves a SIMD."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "neptune-mip_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("leaf_search_expand", "leaf_node_state", "leaf_search_adopt")
_ROWS = {}


def _resources(src):
    if src in _ROWS:
        return _ROWS[src]
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c", os.path.join(CSRC, src),
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=900).stderr
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*([A-Za-z /\[\]]+?): (.+?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            cur = rows.setdefault(v, {})
        elif cur is not None:
            cur[k] = v
    _ROWS[src] = rows
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("kernel", KERNELS)
def test_leaf_search_kernels_use_no_scratch(kernel):
    rows = _resources("nep_leaf_search.hip")
    names = [n for n in rows if re.fullmatch(rf"_ZN3nep{len(kernel)}{kernel}E.*", n)]
    assert len(names) == 1, (kernel, sorted(rows))
    r = rows[names[0]]
    print(kernel, r)
    assert int(r["ScratchSize [bytes/lane]"]) == 0, (kernel, r)
    assert int(r.get("VGPRs Spill", "0")) == 0 and int(r.get("SGPRs Spill", "0")) == 0, (kernel, r)
    assert int(r["VGPRs"]) <= 64, (kernel, r)      # (8 waves a SIMD; DESIGN.md §7 "Native search" states the counts)
