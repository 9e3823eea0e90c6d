"""What the compiler made of fb_fused_kernel (csrc/fused_block.hip), from hipcc's own report
(-Rpass-analysis=kernel-resource-usage; cross-compiles without a GPU, with the Makefile's flags):

* no scratch in any instantiation the launcher selects by default -- the kernel's waits are counted vmcnt, and scratch
  traffic enters the count;
* the MID = 64 and MID = 128 instantiations fit four waves per SIMD, i.e. two 8-wave workgroups per CU (their LDS allows
  it as well): the property the stage-1/2 form is built on, pinned against a later compiler or edit."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_inflight_check as chk  # noqa: E402

LDS_PER_CU = 160 * 1024
FIELDS = {"vgprs": "VGPRs", "agprs": "AGPRs", "scratch": r"ScratchSize \[bytes/lane\]", "waves": r"Occupancy \[waves/SIMD\]",
          "lds": r"LDS Size \[bytes/block\]"}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    flags, _ = chk.makefile_flags()
    out = tmp_path_factory.mktemp("fb") / "fused_block.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "--offload-device-only",
                        "-S", os.path.join(chk.CSRC, "fused_block.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    table = {}
    for blk in re.split(r"(?=remark: Function Name:)", r.stderr):
        m = re.match(r"remark: Function Name: \S*fb_fused_kernelILi(\d+)ELi(\d+)ELi(\d+)E", blk)
        if m:
            table[tuple(int(x) for x in m.groups())] = {k: int(re.search(pat + r": (\d+)", blk).group(1)) for k, pat in FIELDS.items()}
    return table


# what fb_shape selects without any switch set: eight waves of one 16-row strip for every MID
DEFAULT = [(64, 1, 8), (128, 1, 8), (256, 1, 8)]


@pytest.mark.parametrize("inst", DEFAULT)
def test_no_scratch_in_the_default_instantiations(usage, inst):
    assert inst in usage, sorted(usage)
    assert usage[inst]["scratch"] == 0, usage[inst]


@pytest.mark.parametrize("inst", [(64, 1, 8), (128, 1, 8)])
def test_stage_1_and_2_instantiations_fit_two_workgroups_per_cu(usage, inst):
    u = usage[inst]
    assert u["waves"] >= 4, u                      # 2 workgroups x 8 waves on 4 SIMDs
    assert u["vgprs"] + u["agprs"] <= 128, u
    assert 2 * u["lds"] <= LDS_PER_CU, u


def test_stage_3_instantiation_keeps_two_waves_per_simd(usage):
    assert usage[(256, 1, 8)]["waves"] >= 2, usage[(256, 1, 8)]
