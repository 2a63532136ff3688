"""Cases for mdec-k3.11 (NOTEBOOK, "mdec-k3.11"): the 12-wavefront shapes of the frame kernel hold the pixel gather's per-lane tables
-- row offset, second-half offset, row shift, the two byte selectors, the row pass's A operand -- in registers across the pass loop
instead of reading them from LDS in every macroblock (the 16-wavefront shapes read them as before, and run the same cases).  The
tables are a function of the frame's width and height, so the cases turn on geometry:

  16x16     one macroblock: all but one wavefront hold no ticket and re-read macroblock (0, 0) through the held registers
  48x16     three macroblocks in one row;  16x48: three in one column (odd counts)
  64x64     sixteen;  256x128: the smallest frame whose passes have a checkpoint in both workgroup shapes
  640x32    the widest row offsets, the luma lanes' row shift at work

each with all three codecs, in both workgroup shapes (32 frames: 16 wavefronts, 600 frames: 12), under one and two launch lanes,
as a launch with one budget and as a launch with a budget per frame, twice on one context (the second launch is warm).  Every
output byte and every result word is compared with the CPU oracle.

The content makes a frame enter the pass loop several times on the held registers: quiet noise, loud noise, full-contrast
macroblocks among flat ones and a non-monotone pattern of tests/mdec_hard_content.py follow each other in a launch, so a frame
starts from a neighbour's answer that is far off; the per-frame budgets are the exact fit of a scale or one 16-bit word short of
one.  At 256x128 the diagnostics instantiation's records are read to see that this happened: a pass stopped at its
checkpoint, a second emitting pass, and (v2, on the frames tests/test_gpu_mdec_sampled_count.py makes for the judge) a pass that
only counts."""
import os

import numpy as np
import pytest

import mdec_hard_content as H
import oracle_lib as O
import test_gpu_mdec_k310 as K
import test_gpu_mdec_sampled_count as S

pytestmark = pytest.mark.gpu

GEOMETRIES = [(16, 16), (48, 16), (16, 48), (64, 64), (256, 128), (640, 32)]
CODECS = [0, 1, 2]
SHAPES = K.SHAPES              # 32 frames: the 16-wavefront shape, 600: the 12-wavefront shape


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def encoder(codec, w, h, cap, env):
    from psxavenc_amd.mdec import MdecEncoder
    env = dict(env, PSXHIP_MDEC_SPLIT_MAX="0")             # the frame kernel, also for the launches small enough for the split kernel
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return MdecEncoder(codec, w, h, max_frame_size=cap, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def launch_twice(torch, codec, *args, **kwargs):
    """test_gpu_mdec_k310.launch_twice with a context of this codec"""
    old = K.encoder
    K.encoder = lambda w, h, cap, env: encoder(codec, w, h, cap, env)
    try:
        return K.launch_twice(torch, *args, **kwargs)
    finally:
        K.encoder = old


def row(codec, name, w, h, frame, budget, kind):
    """a test_gpu_mdec_sampled_count.Row whose expected bytes are the oracle's for this codec"""
    r = S.Row.__new__(S.Row)
    r.name, r.w, r.h, r.frame, r.budget, r.kind, r.p = name, w, h, np.ascontiguousarray(frame), int(budget), kind, None
    out, res, rc = O.mdec_encode(codec, w, h, r.frame[None, :], int(budget))
    assert rc in (0, -2), rc
    r.res = res[0].copy() if rc == 0 else None
    r.stream = out[0, :int(res[0, 1])].copy() if rc == 0 else None
    r.scale = int(res[0, 0]) if rc == 0 else 64
    return r


def contents(w, h):
    pattern = H.dip_macroblocks()[0][0]
    return [("noise +-4", O.synth_frames(w, h, 1, seed=71, amp=4)[0]),
            ("noise +-24", O.synth_frames(w, h, 1, seed=72, amp=24)[0]),
            ("full contrast among flat", K.mb_pattern(w, h, lambda fx, fy: "noise" if (fx + 3 * fy) % 4 == 0 else None, seed=7)),
            ("dip pattern, tiled", H.tile(pattern, w, h, dc_seed=5))]


def cases(codec, w, h):
    """(rows for a launch with a budget per frame, rows for a launch with one budget)"""
    cap = S.CAP
    per_frame, frames = [], contents(w, h)
    needs = [O.mdec_need(codec, w, h, f) for _, f in frames]
    for (name, f), need in zip(frames, needs):
        # the exact fit of scales 2, 7, 12 and 20, and one 16-bit word short of scales 2, 5 and 10 (the answer is then the next coarser
        # scale that fits, and the search has to prove that the finer one does not); the loud frames keep the coarse ones only
        budgets = {(int(need[s]) + 1) & ~1 for s in (2, 7, 12, 20)} | {int(need[s]) - 2 for s in (2, 5, 10)}
        for b in sorted(x for x in budgets if 8 < x <= cap):
            per_frame.append(row(codec, "%s %dx%d at %d" % (name, w, h, b), w, h, f, b, "per-frame"))
    # one budget for all: the quiet noise's exact fit at scale 3 -- the loud frames need far coarser scales (or do not fit at all)
    u = min(max((int(needs[0][3]) + 1) & ~1, 10), cap)
    uniform = [row(codec, "%s %dx%d at %d" % (name, w, h, u), w, h, f, u, "uniform") for name, f in frames]
    assert len(per_frame) >= 8 and len({r.scale for r in uniform}) >= 2, (len(per_frame), [r.scale for r in uniform])
    return per_frame, uniform


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_every_geometry_codec_shape_and_lane_count_gives_the_oracles_bytes(torch_cuda, w, h, codec):
    from psxavenc_amd.mdec import query_geometry
    assert query_geometry(codec, w, h, S.CAP).fits
    per_frame, uniform = S.shared(("k311", codec, w, h), lambda: cases(codec, w, h))
    print("%dx%d codec %d: per-frame answers %s, uniform answers %s" % (w, h, codec, sorted({r.scale for r in per_frame}), [r.scale for r in uniform]))
    for n in SHAPES:
        for lanes in (1, 2):
            launch_twice(torch_cuda, codec, w, h, K.repeat(per_frame, n, 10 * n + lanes), S.CAP, lanes, False)
            # (alternating, not shuffled: every frame's neighbour in time has another answer)
            launch_twice(torch_cuda, codec, w, h, [uniform[i % len(uniform)] for i in range(n)], S.CAP, lanes, True)


def pass_facts(rec):
    """per frame of a diagnostics launch: (a pass was stopped at its checkpoint, emitting passes among the first four, passes that only count)"""
    _, _, _, passes, trace = S.fields(rec)
    first_abort = (rec.astype(np.int64) >> 8) & 0x7F
    stopped = (first_abort != 0) | ((trace & 0x80) != 0).any(axis=1)
    scale = trace & 0x3F
    emitting = ((scale != 0) & ((trace & 0x40) == 0)).sum(axis=1)
    counting = ((scale != 0) & ((trace & 0x40) != 0)).sum(axis=1)
    return stopped, emitting, counting, passes


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("n", SHAPES)
def test_the_pass_loop_is_entered_again_on_held_registers(torch_cuda, n, codec):
    """256x128, neighbours with far-apart answers at one budget, every hint taken (PSXHIP_MDEC_TRUST=1): the records of the diagnostics
    instantiation have to show passes stopped at the checkpoint and second emitting passes -- and the product kernel's bytes, from the
    same rows, are the oracle's (the test above; here the diagnostics instantiation's are compared as well).  v2 also runs the frame
    made to fool this shape's judge, whose warm launch ends on a pass that only counts, and its reverse."""
    w, h = 256, 128
    _, uniform = S.shared(("k311", codec, w, h), lambda: cases(codec, w, h))
    rows = [uniform[i % len(uniform)] for i in range(n)]
    env = {"PSXHIP_MDEC_STATS": "1", "PSXHIP_MDEC_TRUST": "1"}
    rec = launch_twice(torch_cuda, codec, w, h, rows, S.CAP, 1, True, env=env, want_records=True)
    stopped, emitting, counting, passes = pass_facts(rec)
    print("codec %d, %d frames: stopped at the checkpoint %d, two emitting passes and more %d, a pass that only counts %d, passes %s"
          % (codec, n, stopped.sum(), (emitting >= 2).sum(), (counting >= 1).sum(), np.bincount(passes).tolist()))
    assert stopped.any()
    assert ((emitting >= 2) | (stopped & (passes >= 2))).any()
    if codec == 0:
        large = S.shape_of(torch_cuda, n)
        for make, tag in ((S.fooled_row, "fooled"), (S.reverse_row, "reverse")):
            r = S.shared((tag, w, h, large), lambda: make(w, h, large))
            for uniform_budget in (True, False):
                launch_twice(torch_cuda, codec, w, h, [r] * n, S.CAP, 2, uniform_budget)
            rec = launch_twice(torch_cuda, codec, w, h, [r] * n, S.CAP, 1, True, env=env, want_records=True)
            stopped, emitting, counting, passes = pass_facts(rec)
            print("%s: a pass that only counts on %d of %d, passes %s" % (r.name, (counting >= 1).sum(), n, np.bincount(passes).tolist()))
            if tag == "fooled":
                assert (counting >= 1).sum() * 4 >= 3 * n
