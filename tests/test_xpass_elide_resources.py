"""Register budget of the steady-state plain x pass with chunk elision (CPU: hipcc cross-compiles gfx950 with the
compiler's resource remarks): x_pass<CPL 1|2, CHECK=false, INIT=false, FIRST=false, TW 4|8> — the variants that
carry the elision predicate (nep_kernels.hip "Chunk elision") — keep every VGPR in registers, run at no fewer
waves per SIMD and take no more static LDS than before the predicate was added."""
import os

import pytest

from test_kernel_resources import HIPCC, _compile, _resources

# the compiler's occupancy remark [waves/SIMD] and static LDS [bytes/block] of the same variants at commit 873e737
# (the parent of the change that added the elision), taken by compiling that commit once
PARENT_OCCUPANCY = {(1, 4): 5, (1, 8): 5, (2, 4): 5, (2, 8): 5}
PARENT_LDS = {(1, 4): 1152, (1, 8): 2304, (2, 4): 1152, (2, 8): 2304}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_steady_state_pass_keeps_its_registers_and_occupancy():
    rows = _resources(_compile("nep_kernels.hip"))
    for (cpl, tw), occ in PARENT_OCCUPANCY.items():
        name = f"_ZN3nep6x_passILi{cpl}ELb0ELb0ELb0ELi{tw}EEEvNS_10DeviceViewEPKiiiii"
        assert name in rows, name
        r = rows[name]
        print(cpl, tw, r)
        assert int(r.get("VGPRs Spill", "0")) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= occ, (name, r)
        assert int(r["LDS Size [bytes/block]"]) <= PARENT_LDS[(cpl, tw)], (name, r)
