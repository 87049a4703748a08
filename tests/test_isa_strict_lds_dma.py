"""CPU test (hipcc cross-compiles gfx950 without a GPU): the upstream-order item loop (delta_graph_slam_amd/csrc/ndt_strict.h,
strict_items_float, DGS_STRICT_ITEMS = 3) brings the next round's voxel records into a per-wave LDS ring by LDS-DMA
(global_load_lds_dwordx4) while the current round's items run.  That only pays while the kernel keeps two waves per SIMD and
nothing retires the DMA early, so both are asserted on the compiled timed kernel, ndt_strict3_kernel<DIRECT7, fused, with the
double pass, not fixed>:
  * at most 256 VGPRs, no AGPRs, occupancy 2, no more than 96 bytes of scratch, LDS within two workgroups per CU;
  * in each float item loop: the four DMA loads, and between them and the next s_waitcnt vmcnt(0) (the loop's own, before the
    ring is read) the round's point-table ds_reads and no scratch reload (whose vmcnt wait would drain the DMA too).
The bit-for-bit A/B of the old and new loop is a GPU check (bench.py --dump-outputs); this file guards the instruction schedule."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_graph_slam_amd", "csrc")
TIMED = "_ZN3dgs18ndt_strict3_kernelILi2ELb1ELb1ELb0EE"   # <search = DIRECT7, fused, with the double pass, not fixed>


@pytest.fixture(scope="module")
def asm():
    subprocess.check_call(["make", "-C", CSRC, "isa", "-j2"], stdout=subprocess.DEVNULL)
    return open(os.path.join(CSRC, "build", "ndt_align.s")).read()


def _span(text, prefix):
    m = re.search(r"^(%s\w*):" % re.escape(prefix), text, flags=re.M)
    assert m, prefix
    end = text.index(".Lfunc_end", m.end())
    return m.end(), end


def _body(text, prefix):
    start, end = _span(text, prefix)
    return [ln.strip() for ln in text[start:end].splitlines()]


def _resources(text, prefix):
    _, end = _span(text, prefix)
    tail = text[end:end + 4000]
    out = {}
    for key in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy"):
        m = re.search(r"^; %s: (\d+)" % key, tail, flags=re.M)
        assert m, key
        out[key] = int(m.group(1))
    m = re.search(r"^; LDSByteSize: (\d+)", tail, flags=re.M)
    assert m, "LDSByteSize"
    out["LDS"] = int(m.group(1))
    return out


def test_timed_kernel_keeps_two_waves_per_simd(asm):
    r = _resources(asm, TIMED)
    assert r["NumVgprs"] <= 256 and r["NumAgprs"] == 0, r
    assert r["Occupancy"] == 2, r
    assert r["ScratchSize"] <= 96, r
    assert r["LDS"] <= 81920, r   # two workgroups per CU in 160 KiB


def test_item_loops_overlap_the_record_dma_with_the_items(asm):
    ln = _body(asm, TIMED)
    dma = [i for i, x in enumerate(ln) if x.startswith("global_load_lds_dwordx4")]
    # two float item loops (score + gradient, + Hessian), each with a prologue issue and an in-loop issue of four loads
    assert len(dma) == 16, len(dma)
    labels = {m.group(1): i for i, m in enumerate(re.match(r"^(\.LBB\w+):", x) for x in ln) if m}
    groups = [dma[k:k + 4] for k in range(0, 16, 4)]
    for g in groups:
        assert g[-1] - g[0] < 40, "the four loads of a round are not issued together"
    # per loop: the prologue's issue (round 0, right behind the queue), then the loop header, then the in-loop issue (round r + 1)
    in_loop = []
    for pro, g in ((groups[0], groups[1]), (groups[2], groups[3])):
        assert any("Inner Loop Header" in x for x in ln[pro[-1]:g[0]]), "no loop header between the prologue's DMA and the loop's"
        in_loop.append(g)
    for g in in_loop:
        last = g[-1]
        # the round ends at the first branch back above the DMA issue (to the loop's header or latch; exec-mask skips of idle lanes aside)
        hdr = max(i for i in range(g[0]) if "Inner Loop Header" in ln[i])
        back = next(j for j in range(last + 1, len(ln))
                    if re.match(r"^s_(cbranch_scc[01]|cbranch_vccn?z|branch) (\S+)$", ln[j]) and labels.get(ln[j].split()[1], len(ln)) < g[0])
        wait = next((j for j in range(last + 1, back) if re.match(r"^s_waitcnt vmcnt\(0\)$", ln[j])), back)
        between = ln[last + 1:wait]
        assert wait == back, "vmcnt(0) inside the round retires the DMA early: %s" % ln[wait]
        assert any(re.match(r"^ds_read", x) for x in between), "the point table is not read while the DMA is in flight"
        assert not any(x.startswith("scratch_load") for x in between), "a scratch reload (and its vmcnt wait) sits inside the DMA's shadow"
        top = next(j for j in range(hdr, g[0]) if re.match(r"^s_waitcnt vmcnt\(0\)$", ln[j]))
        assert any(re.match(r"^ds_read_b128", x) for x in ln[top:g[0]]), "the ring is not read behind the loop's vmcnt(0)"


def test_fixed_slices_kernel_keeps_two_waves_per_simd(asm):
    # the fixed-slices instantiation runs the plain loop (no ring: its per-slice column sums take that LDS)
    r = _resources(asm, "_ZN3dgs18ndt_strict3_kernelILi2ELb1ELb1ELb1EE")
    assert r["Occupancy"] == 2 and r["LDS"] <= 81920, r
    assert not any(x.startswith("global_load_lds") for x in _body(asm, "_ZN3dgs18ndt_strict3_kernelILi2ELb1ELb1ELb1EE"))
