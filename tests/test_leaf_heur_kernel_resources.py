"""Resources of the per-round repair's kernels (CPU: hipcc cross-compiles gfx950 with the compiler's resource remarks),
in the manner of tests/test_leaf_kernel_resources.py: leaf_open_lists, leaf_repair_count and leaf_repair_dev use no
scratch — the move loop's search is a chain of dependent gathers, and a spill would add memory round trips to every
candidate.  (Scalar registers that spill go to lanes of a vector register, not to memory; they are not counted.)"""
import os
import re

import pytest

from test_leaf_kernel_resources import HIPCC, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_repair_kernels_use_no_scratch():
    rows = _resources("nep_leaf_heur.hip")
    for kernel in ("leaf_open_lists", "leaf_repair_count", "leaf_repair_dev"):
        names = [n for n in rows if re.fullmatch(rf"_ZN3nep{len(kernel)}{kernel}E.*", n)]
        assert len(names) == 1, (kernel, sorted(rows))
        r = rows[names[0]]
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (kernel, r)
        assert int(r.get("VGPRs Spill", "0")) == 0, (kernel, r)
