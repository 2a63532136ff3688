"""mdec-k3.11: the 12-wavefront shapes of the frame kernel hold the pixel gather's per-lane tables in registers across the pass
loop; the 16-wavefront shapes were left alone (NOTEBOOK, "mdec-k3.11").  Read from
the listing of the six product (stats off) instantiations of the frame kernel, with the flags and the loop finder of
tests/test_kernel_resources.py, in the innermost loop around the third v_mfma (the pass loop's macroblock):

(a) a shape that took the change has at least one LDS read fewer there than its parent had (both table reads are gone: the
    listing has the parent's count minus two);
(b) a shape that was left alone has the parent's count;
(c) between the inline s_load_dwordx16 of the column coefficients and the v_mfma behind it nothing waits on lgkmcnt: that counter
    counts scalar loads too, and a wait there would wait for the very load the row pass is there to hide;
(d) the whole kernel has no scratch, no spilled vector register, and at most 80 / 128 vector registers (12 / 16 wavefronts).

The parent's counts were read from the listing of commit 326fa6b ("Readers' host layer: a plan without HIP, one read-to-host
skeleton", kernel revision mdec-k3.10), built with the same flags."""
import re
import shutil

import pytest

import test_kernel_resources as R

# (codec, wavefronts): ds_read* instructions in the innermost loop around the third v_mfma, at commit 326fa6b
PARENT_DS_READS = {(0, 12): 17, (0, 16): 17, (1, 12): 70, (1, 16): 70, (2, 12): 70, (2, 16): 70}
# ... and how many of them a shape that took the change must have lost at least (0: the shape was left alone)
TOOK = {(0, 12): 1, (0, 16): 0, (1, 12): 1, (1, 16): 0, (2, 12): 1, (2, 16): 0}

_cache = {}


def product_shapes():
    if not _cache:
        use = R._resource_usage("mdec_kernels.hip")
        funcs = R._functions(R._listing("mdec_kernels.hip"))
        for name, lines in funcs.items():
            m = re.search(r"mdec_encode_frames_kernelILi(\d)ELi(\d+)ELi\d+ELb0EEE", name)
            if m:
                _cache[(int(m.group(1)), int(m.group(2)))] = (lines, use[name])
    assert sorted(_cache) == sorted(PARENT_DS_READS), sorted(_cache)
    return _cache


def pass_loop(lines):
    sites = [i for i, ln in enumerate(lines) if "v_mfma" in ln]
    assert len(sites) == 3, sites
    a, b = R._innermost_loop(lines, sites[2])
    return a, b, sites[2]


@pytest.mark.skipif(not shutil.which(R.HIPCC), reason="hipcc not installed")
def test_the_pass_loop_reads_the_gather_tables_no_more():
    for shape, (lines, _) in product_shapes().items():
        a, b, _ = pass_loop(lines)
        reads = sum(1 for ln in lines[a:b + 1] if re.match(r"\s+ds_read", ln))
        print(shape, "ds_read* in the loop of lines %d..%d: %d (parent %d)" % (a, b, reads, PARENT_DS_READS[shape]))
        if TOOK[shape]:
            assert reads <= PARENT_DS_READS[shape] - TOOK[shape], (shape, reads)
        else:
            assert reads == PARENT_DS_READS[shape], (shape, reads)


@pytest.mark.skipif(not shutil.which(R.HIPCC), reason="hipcc not installed")
def test_nothing_waits_for_lds_or_scalar_loads_between_the_coefficient_load_and_the_row_pass():
    for shape, (lines, _) in product_shapes().items():
        a, b, mfma = pass_loop(lines)
        loads = [i for i in range(a, b + 1) if "s_load_dwordx16" in lines[i]]
        assert len(loads) == 1, (shape, loads)
        load = loads[0]
        # (the scheduler is free to put the matrix instruction in front of the load: then nothing stands between them at all)
        between = lines[load + 1:mfma] if load < mfma else []
        assert len(between) < 8, (shape, load, mfma)          # the load is issued where the row pass starts, not somewhere far off
        waits = [ln.strip() for ln in between if "s_waitcnt" in ln and "lgkmcnt" in ln]
        assert not waits, (shape, waits)
        if load > mfma:
            assert load - mfma < 8, (shape, load, mfma)


@pytest.mark.skipif(not shutil.which(R.HIPCC), reason="hipcc not installed")
def test_product_shapes_hold_the_tables_without_scratch():
    for (codec, waves), (_, u) in product_shapes().items():
        assert u["ScratchSize"] == "0" and u["VGPRs Spill"] == "0", ((codec, waves), u)
        assert int(u["VGPRs"]) <= (80 if waves == 12 else 128), ((codec, waves), u)
