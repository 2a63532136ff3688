"""Cases written for the instruction work of mdec-k3.10 on the v2 frame kernel (NOTEBOOK, "mdec-k3.10").  What shipped is the merge
with 8 instead of 16 lanes per macroblock; tried and dropped were the macroblock's sums added in one place behind the join of its
arms and the chunk's run and table offset computed on 4 x the scan position -- the latter gave wrong bytes on the device, and these
cases are what caught it.  They cover all three: the uncounted macroblock's arm on a warm launch, escape codes and lists of several
chunks, the DC quantiser's ends and ties, and the merge on short, long and uneven streams (one turn of 8 lanes, several, and both
in one round) and over several image tiles.  Every case is compared with the CPU oracle, every output byte and every result word,
on two launches of one context (the second is warm) and under one and two launch lanes.

Geometry: 256x128 (128 macroblocks) is the smallest frame whose passes have a checkpoint -- and with it the flag that stops the
count -- in both workgroup shapes; 32 frames run the 16-wavefront shape, 600 the 12-wavefront shape.  The merge cases also run
64x64, and every row runs both as a launch with ONE budget for all frames and as a launch with a budget per frame (a device tensor;
the context is then made for a larger budget than any row's)."""
import os

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_mdec_sampled_count as S

pytestmark = pytest.mark.gpu

FILL = S.FILL
SHAPES = [32, 600]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def encoder(w, h, cap, env):
    from psxavenc_amd.mdec import MdecEncoder
    env = dict(env, PSXHIP_MDEC_SPLIT_MAX="0")
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        return MdecEncoder(0, w, h, max_frame_size=cap, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def launch_twice(torch, w, h, rows, cap, lanes, uniform, env=None, want_records=False):
    """the rows as one launch, twice on one context; uniform: the launch's single budget (all rows must have it), else a budget per
    frame from a device tensor.  Both launches are compared with the oracle; returns the second launch's stats records if asked"""
    enc = encoder(w, h, cap, env or {})
    if lanes > 1:
        enc.set_lanes(2)
    d_frames = torch.from_numpy(np.stack([r.frame for r in rows])).to("cuda:0")
    if uniform:
        assert all(r.budget == rows[0].budget for r in rows)
        budgets = rows[0].budget
    else:
        budgets = torch.tensor([r.budget for r in rows], dtype=torch.int32, device="cuda:0")
    outs, rec = [], None
    for k in range(2):
        d_out = torch.full((len(rows), cap), FILL, dtype=torch.uint8, device="cuda:0")
        outs.append(enc.encode_frames_device(d_frames, budgets, d_out=d_out))
        if want_records:
            enc.fence()
            torch.cuda.synchronize()
            rec = S.records(enc, len(rows))
    enc.fence()
    torch.cuda.synchronize()
    assert enc.watchdog() == 0
    enc.close()
    for k, (o, q) in enumerate(outs):
        S.compare(rows, o.cpu().numpy(), q.cpu().numpy(), "%dx%d, %d rows, %d lane(s), %s budget, launch %d"
                  % (w, h, len(rows), lanes, "one" if uniform else "per-frame", k))
    return rec


def mb_dwords(row):
    """dwords of the oracle's stream per macroblock, on average"""
    return (row.stream.size - 8) / 4.0 / ((row.w // 16) * (row.h // 16))


# ---------------------------------------------------------------- content
def nv21(w, h, luma, chroma):
    return np.concatenate([np.asarray(luma, np.uint8).reshape(h, w).ravel(), np.asarray(chroma, np.uint8).reshape(h // 2, w).ravel()])


def flat(w, h, v):
    return nv21(w, h, np.full((h, w), v), np.full((h // 2, w), v))


def mb_pattern(w, h, fn, seed=0):
    """per macroblock (fx, fy): fn -> None (mid grey, flat), an int (flat at that value) or "noise" (every sample 0 or 255)"""
    rng = np.random.default_rng(seed)
    lu, ch = np.full((h, w), 128, np.uint8), np.full((h // 2, w), 128, np.uint8)
    for fy in range(h // 16):
        for fx in range(w // 16):
            v = fn(fx, fy)
            if v is None:
                continue
            if isinstance(v, str):
                lu[fy * 16:fy * 16 + 16, fx * 16:fx * 16 + 16] = rng.integers(0, 2, (16, 16)) * 255
                ch[fy * 8:fy * 8 + 8, fx * 16:fx * 16 + 16] = rng.integers(0, 2, (8, 16)) * 255
            else:
                lu[fy * 16:fy * 16 + 16, fx * 16:fx * 16 + 16] = v
                ch[fy * 8:fy * 8 + 8, fx * 16:fx * 16 + 16] = 255 - v if (fx + fy) & 1 else v
    return nv21(w, h, lu, ch)


def fit_budget(w, h, frame, scale, cap):
    """the smallest even budget at which the oracle's answer for this frame is `scale`"""
    need = O.mdec_need(0, w, h, frame)
    b = (int(need[scale]) + 1) & ~1
    assert 8 < b <= cap, (b, cap)
    return b


def repeat(rows, n, seed):
    rng = np.random.default_rng(seed)
    return [rows[i] for i in rng.permutation(np.arange(n) % len(rows))]


# ---------------------------------------------------------------- (a) the uncounted path
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", SHAPES)
def test_noise_far_over_the_limit_takes_the_uncounted_path_when_warm(torch_cuda, n, lanes):
    """noise +-4 with need(p - 1) = 1.7 x limit: the warm launch starts every frame from the answer, stops counting at the mark and
    runs the rest of the frame through the uncounted macroblock's arm -- the headline's hot path.  The product
    kernel's bytes first, then the diagnostics instantiation's, whose records say which path ran."""
    w, h = 256, 128
    large = S.shape_of(torch_cuda, n)
    base = S.shared(("ratio", w, h, large), lambda: S.ratio_rows(w, h, large, 8, seed=40 + w))
    row = [r for r in base if r.kind == 1.7][0]
    rows = [row] * n
    print("%s: budget %d, %.1f dwords per macroblock" % (row.name, row.budget, mb_dwords(row)))
    for uniform in (True, False):
        launch_twice(torch_cuda, w, h, rows, S.CAP, lanes, uniform)
    rec = launch_twice(torch_cuda, w, h, rows, S.CAP, lanes, True, env={"PSXHIP_MDEC_STATS": "1", "PSXHIP_MDEC_TRUST": "1"}, want_records=True)
    guess, stopped, answer, passes, _ = S.fields(rec)
    print("warm: first guess right on %d of %d, passes %s, counting stopped on %d" % ((guess == row.p).sum(), n, np.bincount(passes).tolist(), stopped.sum()))
    assert (answer == row.p).all() and (guess == row.p).all()
    assert stopped.all() and (passes == 1).all()


# ---------------------------------------------------------------- (b) escape codes and lists of several chunks
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", SHAPES)
def test_full_contrast_at_scales_1_and_2(torch_cuda, n, lanes):
    """every fourth macroblock full-contrast noise, the rest flat, at the budgets that make the answer 1 and 2: levels far past the
    table's 41 (escape codes and their run field) and lists of six chunks (the carries across chunks)"""
    w, h, cap = 256, 128, 65536
    from psxavenc_amd.mdec import query_geometry
    assert query_geometry(0, w, h, cap).fits

    def make():
        rows = []
        for seed in (1, 2):
            f = mb_pattern(w, h, lambda fx, fy: "noise" if (fx + 3 * fy) % 4 == 0 else None, seed=seed)
            for scale in (1, 2):
                rows.append(S.Row("full contrast #%d at scale %d" % (seed, scale), w, h, f, fit_budget(w, h, f, scale, cap), "contrast", scale))
                assert rows[-1].scale == scale
        return rows
    base = S.shared(("contrast", w, h), make)
    launch_twice(torch_cuda, w, h, repeat(base, n, n + lanes), cap, lanes, False)


# ---------------------------------------------------------------- (c) the DC quantiser's ends and ties
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", SHAPES)
def test_flat_frames_and_checkerboards(torch_cuda, n, lanes):
    """flat at 0 and at 255, a checkerboard of both, and every grey level in turn: the DC term at both ends of its clamp and on the
    rounding ties 16 m + 8 of both signs"""
    w, h = 256, 128

    def make():
        nx = w // 16
        frames = [flat(w, h, 0), flat(w, h, 255),
                  mb_pattern(w, h, lambda fx, fy: 255 * ((fx + fy) & 1)),
                  mb_pattern(w, h, lambda fx, fy: (2 * (fy * nx + fx)) & 255),
                  mb_pattern(w, h, lambda fx, fy: (2 * (fy * nx + fx) + 1) & 255)]
        return [S.Row("flat / checkerboard #%d" % i, w, h, f, 4096, "flat") for i, f in enumerate(frames)]
    base = S.shared(("flat", w, h), make)
    rows = repeat(base, n, n + lanes)
    for uniform in (True, False):
        launch_twice(torch_cuda, w, h, rows, S.CAP, lanes, uniform)


# ---------------------------------------------------------------- (d) the merge
MERGE_CAP = 16384         # the merge cases' contexts: room for 24 dwords per macroblock at 256x128


def merge_rows(w, h):
    nmb = (w // 16) * (h // 16)
    rows = {}
    # short streams: 3 .. 7 dwords per macroblock
    f = O.synth_frames(w, h, 1, seed=5, amp=6)[0]
    b = 8 + 4 * 5 * nmb
    rows["short"] = S.Row("noise +-6 %dx%d at %d" % (w, h, b), w, h, f, b, "short")
    # long ones: 9 .. 40
    f = O.synth_frames(w, h, 1, seed=6, amp=24)[0]
    b = 8 + 4 * 24 * nmb
    rows["long"] = S.Row("noise +-24 %dx%d at %d" % (w, h, b), w, h, f, b, "long")
    # a few long streams among short ones, in a budget that leaves a macroblock fewer than eight dwords
    f = mb_pattern(w, h, lambda fx, fy: "noise" if (fx + 5 * fy) % 8 == 0 else 16 * ((fx + fy) & 7), seed=3)
    b = 8 + 4 * 6 * nmb
    rows["uneven"] = S.Row("uneven %dx%d at %d" % (w, h, b), w, h, f, b, "uneven")
    for k, r in rows.items():
        assert r.res is not None, k
    return rows


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("w,h,n", [(64, 64, 32), (64, 64, 600), (256, 128, 32), (256, 128, 600)])
def test_merge_of_short_long_and_uneven_streams(torch_cuda, w, h, n, lanes):
    """3 .. 7 dwords per macroblock (at most one turn of 8 lanes), 9 .. 40 (more than one turn of 16), and a few long streams among
    short ones at a budget that averages six"""
    rows = S.shared(("merge", w, h), lambda: merge_rows(w, h))
    for kind in ("short", "uneven", "long"):
        r = rows[kind]
        d = mb_dwords(r)
        print("%s: scale %d, %.1f dwords per macroblock" % (r.name, r.scale, d))
        assert (3 <= d <= 7) if kind != "long" else (9 <= d <= 40), (kind, d)
        for uniform in (True, False):
            launch_twice(torch_cuda, w, h, [r] * n, MERGE_CAP, lanes, uniform)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("w,h", [(64, 64), (256, 128)])
def test_merge_over_several_image_tiles(torch_cuda, w, h, lanes):
    """a budget the frame image of which is assembled one tile at a time, and a stream that reaches into the later tiles"""
    from psxavenc_amd.mdec import query_geometry
    cap = None
    for c in (49152, 65536, 98304, 131072, 163840, 196608):
        g = query_geometry(0, w, h, c)
        if g.fits and g.image_tile_bytes < c:
            cap = c
            break
    assert cap is not None, "no budget at %dx%d is assembled in tiles" % (w, h)

    def make():
        f = mb_pattern(w, h, lambda fx, fy: "noise", seed=9)
        r = S.Row("full contrast everywhere %dx%d at %d" % (w, h, cap), w, h, f, cap, "tiles")
        assert r.res is not None and r.stream.size > g.image_tile_bytes, (r.stream.size, g.image_tile_bytes)
        return r
    r = S.shared(("tiles", w, h), make)
    print("%s: image tile %d bytes, stream %d bytes, scale %d" % (r.name, g.image_tile_bytes, r.stream.size, r.scale))
    for n in SHAPES if w == 64 else (32,):
        launch_twice(torch_cuda, w, h, [r] * n, cap, lanes, True)
