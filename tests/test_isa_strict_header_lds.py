"""CPU test (hipcc cross-compiles gfx950 without a GPU): the item-compacted upstream-order NDT kernel multiplies every point with the
pair's angle tables (strict_point_tables / strict_point_tables_hd in delta_graph_slam_amd/csrc/ndt_strict.h).  Read through the NdtPair
record, those wave-uniform values were fetched again from L2 for every 64 points -- 38 vector loads in groups behind s_waitcnt vmcnt, on
top of the point and its seven cell2vox look-ups.  The kernel now keeps them in a per-workgroup LDS block (StrictHeader<true>) and this
file holds the compiled timed kernel, ndt_strict3_kernel<DIRECT7, fused, with the double pass, not fixed>, to it, instruction stream only:

  * the sub-tile loop -- the innermost loop that holds the seven consecutive cell2vox global_load_dword of the bounds-tested
    neighbourhood -- contains, LDS-DMA aside, no vector load from global memory but the point (one load of its three or four words) and the
    look-ups.  The body holds BOTH alternatives of strict_neighbourhood, exec-masked one after the other: the bounds-tested one (the seven
    single-dword loads) and the interior one (base pointer + fixed offsets, which the compiler may merge into wider loads).  A code path
    through the body takes one of them, so per path that is at most 1 + 7 loads; statically: one point load, the run of seven, and at
    most seven more loads of at most seven more dwords.  (The parent commit's listing: 50 loads in this loop, 38 of them the header.)
  * the header block is read by ds_read inside that loop (not hoisted into registers: the kernel sits at 256 VGPRs);
  * the fixed-slices DIRECT7 instantiation, which keeps reading the record (its LDS is spoken for, and it is the bit reference of the GPU
    test), still meets what tests/test_isa_strict_lds_dma.py states for it: occupancy 2, LDS for two workgroups per CU, no LDS-DMA.
The bit-for-bit comparison of the two is a GPU check (tests/test_strict_header_lds_gpu.py)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_graph_slam_amd", "csrc")
TIMED = "_ZN3dgs18ndt_strict3_kernelILi2ELb1ELb1ELb0EE"   # <search = DIRECT7, fused, with the double pass, not fixed>
FIXED = "_ZN3dgs18ndt_strict3_kernelILi2ELb1ELb1ELb1EE"   # the same with fixed slices
LABEL = re.compile(r"^\.L(BB\w+):")
VLOAD = re.compile(r"^(global|buffer|flat)_load_")


@pytest.fixture(scope="module")
def asm():
    subprocess.check_call(["make", "-C", CSRC, "isa", "-j2"], stdout=subprocess.DEVNULL)
    return open(os.path.join(CSRC, "build", "ndt_align.s")).read()


def _span(text, prefix):
    m = re.search(r"^(%s\w*):" % re.escape(prefix), text, flags=re.M)
    assert m, prefix
    return m.end(), text.index(".Lfunc_end", m.end())


def _body(text, prefix):
    start, end = _span(text, prefix)
    return [ln.strip() for ln in text[start:end].splitlines()]


def _is_dma(x):
    return x.startswith("global_load_lds") or bool(re.search(r"\blds\b", x))


def _dwords(x):
    m = re.match(r"^\w+_load_dword(x(\d))?\b", x)
    assert m, x
    return int(m.group(2) or 1)


def sub_tile_loop(ln):
    """The lines of the innermost loop around the run of seven consecutive single-dword global loads (no other vector load between them),
    from the compiler's own loop annotations: the labelled blocks marked `in Loop: Header=H` (and H itself), each from its label to the next
    label, cut where control cannot fall through (s_branch) or leaves the loop by falling out of a back-edge to H."""
    loads = [i for i, x in enumerate(ln) if VLOAD.match(x) and not _is_dma(x)]
    runs = []
    k = 0
    while k < len(loads):
        j = k
        while j < len(loads) and re.match(r"^global_load_dword ", ln[loads[j]]):
            j += 1
        if j - k >= 7:
            runs.append(loads[k:j])
        k = max(j, k + 1)
    labels = [i for i, x in enumerate(ln) if LABEL.match(x)]

    def note(lab):   # the label's loop annotation: its own comment and the comment lines right below it
        out, i = ln[lab], lab + 1
        while i < len(ln) and ln[i].startswith(";") and "Loop" in ln[i]:
            out, i = out + " " + ln[i], i + 1
        return out

    def header_of(i):
        lab = max(l for l in labels if l <= i)
        m = re.search(r"in Loop: Header=(BB\w+)", note(lab))
        if m:
            return m.group(1)
        assert "Loop Header" in note(lab), "line %d is in no loop: %s" % (i, note(lab))
        return LABEL.match(ln[lab]).group(1)

    # the neighbourhood's run: seven loads, all in blocks of one loop, inside the tile loop (depth >= 3: slice loop, tile loop, sub-tile loop)
    cands = [r for r in runs if len(r) == 7 and len({header_of(i) for i in r}) == 1]
    assert len(cands) == 1, "runs of seven single-dword loads: %s" % [(r[0], len(r)) for r in runs]
    run = cands[0]
    hdr = header_of(run[0])
    body = []
    for n, lab in enumerate(labels):
        name = LABEL.match(ln[lab]).group(1)
        assert name == hdr or not re.search(r"Parent Loop %s\b" % hdr, note(lab)), "a loop nested inside the sub-tile loop: not the innermost"
        if name != hdr and not re.search(r"in Loop: Header=%s\b" % hdr, note(lab)):
            continue
        end = labels[n + 1] if n + 1 < len(labels) else len(ln)
        for i in range(lab, end):
            body.append(i)
            if re.match(r"^s_branch ", ln[i]) or ln[i].startswith("s_endpgm"):
                break
            if re.match(r"^s_cbranch_\w+ \.L%s$" % hdr, ln[i]) and i + 1 < end and ln[i + 1].startswith("; %bb."):
                break
    assert all(i in set(body) for i in run)
    return hdr, body, run


def test_sub_tile_loop_loads_the_point_and_its_look_ups_only(asm):
    ln = _body(asm, TIMED)
    hdr, body, run = sub_tile_loop(ln)
    loads = [i for i in body if VLOAD.match(ln[i]) and not _is_dma(ln[i])]
    point = loads[:1]   # the body's first load: x y z (w) of the source point, through the pair's source pointer
    other = [i for i in loads if i not in point and i not in run]
    print("sub-tile loop %s: %d lines, %d vector loads from global memory (point %d, bounds-tested look-ups %d, interior look-ups %d in %d dwords)"
          % (hdr, len(body), len(loads), len(point), len(run), len(other), sum(_dwords(ln[i]) for i in other)))
    for i in loads:
        print("   ", i, ln[i])
    assert len(point) == 1 and re.match(r"^(flat|global)_load_dwordx[34] ", ln[point[0]]) and point[0] < run[0], [ln[i] for i in point]
    # a path takes the bounds-tested look-ups (the run of seven) or the interior ones: at most 1 + 7 loads either way
    assert len(run) == 7
    assert len(other) <= 7 and sum(_dwords(ln[i]) for i in other) <= 7, [ln[i] for i in other]
    assert not any(ln[i].startswith("scratch_load") for i in body), "a scratch reload inside the sub-tile loop"


def test_header_block_is_read_from_lds_inside_the_sub_tile_loop(asm):
    ln = _body(asm, TIMED)
    _, body, _ = sub_tile_loop(ln)
    reads = [ln[i] for i in body if ln[i].startswith("ds_read")]
    f32 = [x for x in reads if re.match(r"^ds_read2?_b32\b", x)]
    f64 = [x for x in reads if re.match(r"^ds_read2?_b64\b", x)]
    print("ds_read in the sub-tile loop: %d (b32 forms %d, b64 forms %d)" % (len(reads), len(f32), len(f64)))
    # the float tables: 21 + 15 entries enter an evaluation with the Hessian (the z entries that are exact zeros are skipped);
    # the double vectors: jang_d's 8 rows and hang_d's rows 6..14, three entries each (rows 0..5 are rebuilt from jang_d's products at item time)
    assert sum(2 if x.startswith("ds_read2") else 1 for x in f32) >= 36, f32
    assert sum(2 if x.startswith("ds_read2") else 1 for x in f64) >= 51, f64


def test_fixed_slices_kernel_reads_the_record_and_keeps_its_limits(asm):
    ln = _body(asm, FIXED)
    _, end = _span(asm, FIXED)
    tail = asm[end:end + 4000]
    res = {k: int(re.search(r"^; %s: (\d+)" % k, tail, flags=re.M).group(1)) for k in ("Occupancy", "LDSByteSize", "NumVgprs")}
    assert res["Occupancy"] == 2 and res["LDSByteSize"] <= 81920 and res["NumVgprs"] <= 256, res
    assert not any(x.startswith("global_load_lds") for x in ln)
    _, body, _ = sub_tile_loop(ln)
    assert not any(ln[i].startswith("ds_read") for i in body), "the fixed-slices instantiation has no LDS header block"
    loads = [i for i in body if VLOAD.match(ln[i]) and not _is_dma(ln[i])]
    assert len(loads) > 1 + 7 + 7, "the fixed-slices instantiation reads the angle tables from the record"
