"""CPU test (hipcc cross-compiles gfx950 without a GPU): the item-compacted upstream-order NDT kernel that the benchmark times,
ndt_strict3_kernel<DIRECT7, fused, with the double pass, slices dealt per launch> (delta_graph_slam_amd/csrc/ndt_strict.h), sits at
256 VGPRs and two waves per SIMD, where there is no AGPR room to spill into: every spilled VGPR is a scratch-memory round trip on the
vector memory path, next to the LDS-DMA of the voxel records.  The kernel is kept free of them -- the wave's number, its tile stride
and gd2 are scalars, per-lane LDS addresses are base + lane offset at their use, the solver's six angles are chosen by selects instead
of a stack array read at a per-lane offset -- and this test holds the code object's metadata to that: no private segment, no spilled
VGPR, at most 256 VGPRs, LDS for two workgroups per CU.  Only the metadata is read, no instruction stream."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_graph_slam_amd", "csrc")
TIMED = "_ZN3dgs18ndt_strict3_kernelILi2ELb1ELb1ELb0EE"   # <DIRECT7, fused, with the double pass, not fixed slices>
FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def metadata():
    subprocess.check_call(["make", "-C", CSRC, "build/ndt_align.s"], stdout=subprocess.DEVNULL)   # as tests/test_isa_handoff.py: an existing build is reused
    text = open(os.path.join(CSRC, "build", "ndt_align.s")).read()
    text = text[text.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"^  - (?=\.)", text, flags=re.M) if re.search(r"^\s*\.name:\s+%s" % re.escape(TIMED), e, flags=re.M)]
    assert len(entries) == 1, "metadata entry of the timed instantiation"
    out = {}
    for f in FIELDS:
        m = re.search(r"^\s*\.%s:\s+(\d+)\s*$" % f, entries[0], flags=re.M)
        assert m, f
        out[f] = int(m.group(1))
    return out


def test_timed_kernel_has_no_scratch_and_no_spilled_vgprs(metadata):
    print(metadata)
    assert metadata["private_segment_fixed_size"] == 0
    assert metadata["vgpr_spill_count"] == 0


def test_timed_kernel_keeps_two_workgroups_per_cu(metadata):
    assert metadata["vgpr_count"] <= 256          # two waves per SIMD
    assert metadata["group_segment_fixed_size"] <= 81920   # two workgroups in a CU's 160 KiB of LDS
