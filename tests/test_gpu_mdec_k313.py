"""Cases for mdec-k3.13 (NOTEBOOK, "mdec-k3.13"): the frame kernel's coefficient tile and code list hold a coefficient DOUBLED, with
the accumulator's next bit below it (v' = 2 n + b; an entry keeps 2 n), the list's thresholds and the quantisers' reciprocals are
scaled to match, the chunk takes an entry's scan position with one shift, a one-chunk list's first lane gets its predecessor from
the DPP's zero fill, and the code lengths' prefix sum is six DPP adds.

Every output byte and every result word is compared with the CPU oracle, on two launches of one context (cold and warm), for all
three codecs, in both workgroup shapes (32 frames: 16 wavefronts, 600 frames: 12, as tests/test_gpu_mdec_k311.py picks them), under
one and two launch lanes, as a launch with one budget and as a launch with a budget per frame.

Geometry: 16x16 (one macroblock: first and last at once), 48x16, 16x48, 64x64, 256x128, and 640x32 -- the latter also with a budget
whose frame image is assembled over several tiles.

Content: flat frames of 0, 128 and 255; noise +-4, +-8 and +-40 (coefficients of both signs and both values of the bit below, on and
off the quantiser's ties and the list's thresholds); per-pixel checkerboards and blocks that are the sign pattern of one basis
function each, at full contrast (the largest coefficients a block can have; escape codes at the fine scales); a frame whose first
macroblock in encode order has the longest stream and whose last has the shortest.  Lists of more than 64 and more than 128 entries
(the recompaction and the dense arm) at 256x128, and the frame of tests/test_gpu_mdec_sampled_count.py whose warm launch needs a pass
that only counts."""
import numpy as np
import pytest

import oracle_lib as O
import test_gpu_mdec_k310 as K
import test_gpu_mdec_k311 as K11
import test_gpu_mdec_k312 as K12
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


# ---------------------------------------------------------------- content
def checker_frame(w, h):
    """every plane a per-pixel checkerboard of 0 and 255 (Cb inverted): all of a block's energy in its highest frequency"""
    lu = ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255
    ch = np.zeros((h // 2, w), np.int64)
    c = ((np.arange(h // 2)[:, None] + np.arange(w // 2)[None, :]) & 1) * 255
    ch[:, 0::2] = c
    ch[:, 1::2] = 255 - c
    return K.nv21(w, h, lu, ch)


def basis_frame(w, h, first):
    """block i of the frame (six per macroblock, raster order) is the sign pattern of basis function (first + i) % 64 at full
    contrast, inverted for every other run of 64"""
    x = (2 * np.arange(8) + 1) * np.pi / 16
    lu, ch = np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)
    i = first
    for fy in range(h // 16):
        for fx in range(w // 16):
            for b in range(6):
                u, v = (i % 64) % 8, (i % 64) // 8
                pos = np.cos(x * v)[:, None] * np.cos(x * u)[None, :] >= 0
                if (i // 64) & 1:
                    pos = ~pos
                K12.block_view(lu, ch, fx, fy, b)[:, :] = np.where(pos, 255, 0)
                i += 1
    return K.nv21(w, h, lu, ch)


def long_first_short_last_frame(w, h):
    """quiet noise; the first macroblock in encode order -- (0, 0) -- full-contrast noise, the last -- the bottom right one -- flat"""
    nx, ny = w // 16, h // 16
    f = O.synth_frames(w, h, 1, seed=313, amp=8)[0]
    f = S._paste(f, K.mb_pattern(w, h, lambda fx, fy: "noise", seed=13), w, h, [0])
    if nx * ny > 1:
        f = S._paste(f, K.flat(w, h, 128), w, h, [nx * ny - 1])
    return f


def contents(w, h):
    out = [("flat %d" % v, K.flat(w, h, v)) for v in (0, 128, 255)]
    out += [("noise +-%d" % amp, O.synth_frames(w, h, 1, seed=130 + amp, amp=amp)[0]) for amp in (4, 8, 40)]
    out += [("checkerboard", checker_frame(w, h)), ("basis patterns", basis_frame(w, h, 0)), ("basis patterns, inverted", basis_frame(w, h, 64 + 29)),
            ("long first, short last", long_first_short_last_frame(w, h))]
    return out


def cases(codec, w, h):
    """(rows for a launch with a budget per frame, rows for a launch with one budget), as tests/test_gpu_mdec_k312.py makes them"""
    cap = S.CAP
    frames = contents(w, h)
    needs = {name: O.mdec_need(codec, w, h, f) for name, f in frames}
    per_frame = []
    for name, f in frames:
        need = needs[name]
        # the exact fit of scales 1, 2, 4, 9 and 20 and one 16-bit word short of scale 3: the three finest that the context has room for
        budgets = sorted({(int(need[s]) + 1) & ~1 for s in (1, 2, 4, 9, 20)} | {int(need[3]) - 2})
        for b in [x for x in budgets if 8 < x <= cap][-3:]:
            per_frame.append(K11.row(codec, "%s %dx%d at %d" % (name, w, h, b), w, h, f, b, "per-frame"))
    u = min(max((int(needs["noise +-8"][3]) + 1) & ~1, 10), cap)
    uniform = [K11.row(codec, "%s %dx%d at %d" % (name, w, h, u), w, h, f, u, "uniform") for name, f in frames]
    # conditions on the inputs, from the oracle alone: the largest coefficients are there, of both signs, and inside the tile's range
    top = max(int(np.abs(O.mdec_coefs(w, h, f)[:, :, 1:].astype(np.int64)).max()) for _, f in frames)
    assert 4096 < top <= 8192, top
    return per_frame, uniform, top


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_doubled_coefficients_give_the_oracles_bytes(torch_cuda, w, h, codec):
    from psxavenc_amd.mdec import query_geometry
    assert query_geometry(codec, w, h, S.CAP).fits
    per_frame, uniform, top = S.shared(("k313", codec, w, h), lambda: cases(codec, w, h))
    print("%dx%d codec %d: %d frames, largest AC coefficient %d, per-frame answers %s, uniform answers %s"
          % (w, h, codec, len(uniform), top, sorted({r.scale for r in per_frame}), sorted({r.scale for r in uniform})))
    for n in SHAPES:
        for lanes in (1, 2):
            K11.launch_twice(torch_cuda, codec, w, h, K.repeat(per_frame, n, 13 * n + lanes), S.CAP, lanes, False)
            K11.launch_twice(torch_cuda, codec, w, h, [uniform[i % len(uniform)] for i in range(n)], S.CAP, lanes, True)


# ---------------------------------------------------------------- several image tiles
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("lanes", [1, 2])
def test_a_wide_frame_over_several_image_tiles(torch_cuda, lanes, codec):
    """640x32 at a budget whose frame image is assembled one tile at a time, with streams that reach into the later tiles"""
    from psxavenc_amd.mdec import query_geometry
    w, h = 640, 32
    cap = None
    for c in (16384, 24576, 32768, 49152, 65536, 98304, 131072):
        g = query_geometry(codec, w, h, c)
        if g.fits and g.image_tile_bytes < c:
            cap = c
            break
    assert cap is not None, "no budget at %dx%d is assembled in tiles" % (w, h)

    def make():
        rows = [K11.row(codec, "%s %dx%d at %d" % (name, w, h, cap), w, h, f, cap, "tiles")
                for name, f in (("full contrast everywhere", K.mb_pattern(w, h, lambda fx, fy: "noise", seed=9)),
                                ("checkerboard", checker_frame(w, h)), ("basis patterns", basis_frame(w, h, 7)))]
        assert all(r.res is not None for r in rows) and max(r.stream.size for r in rows) > g.image_tile_bytes, [r.stream.size for r in rows]
        return rows
    rows = S.shared(("k313 tiles", codec, w, h), make)
    print("codec %d: budget %d, image tile %d bytes, streams %s bytes, scales %s"
          % (codec, cap, g.image_tile_bytes, [r.stream.size for r in rows], [r.scale for r in rows]))
    K11.launch_twice(torch_cuda, codec, w, h, [rows[i % len(rows)] for i in range(32)], cap, lanes, True)


# ---------------------------------------------------------------- long lists and escape codes
def long_rows(codec, w, h, cap):
    rows, kinds = [], set()

    def at_scale(name, f, p):
        need = O.mdec_need(codec, w, h, f)
        b = (int(need[p]) + 1) & ~1
        assert 8 < b <= cap, (name, p, b)
        r = K11.row(codec, "%s at scale %d" % (name, p), w, h, f, b, "long")
        assert r.scale == p, (name, p, r.scale)
        return r
    for amp, scales in ((40, (1, 2)), (8, (3,)), (6, (3,))):
        f = O.synth_frames(w, h, 1, seed=330 + amp, amp=amp)[0]
        for p in scales:
            rows.append(at_scale("noise +-%d" % amp, f, p))
            at = K12.list_lengths(w, h, f, p)
            if (at > 128).any():
                kinds.add("an emit list of three chunks and more")
            if p > 1:
                below = K12.list_lengths(w, h, f, p - 1)
                if (below > 128).any():
                    kinds.add("a count list too long to walk: the dense arm")
                if ((below > 64) & (below <= 128) & (at > 64)).any():
                    kinds.add("a count list of two chunks that stays longer than one after the recompaction")
                if ((below > 64) & (below <= 128) & (at <= 64)).any():
                    kinds.add("a count list of two chunks that is one after the recompaction")
    assert len(kinds) == 4, kinds
    # every fourth macroblock full-contrast noise at the budgets of scales 1 and 2: levels far past the table's 41 -- escape codes
    f = K.mb_pattern(w, h, lambda fx, fy: "noise" if (fx + 3 * fy) % 4 == 0 else None, seed=3)
    rows += [at_scale("full contrast among flat", f, p) for p in (1, 2)]
    rc, levels, _, _, _ = O.mdec_decode(w, h, rows[-1].stream)
    assert rc == 0 and int(np.abs(levels[:, 1:].astype(np.int64)).max()) > 41
    return rows


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", SHAPES)
def test_long_lists_and_escape_codes(torch_cuda, n, lanes, codec):
    w, h, cap = 256, 128, 65536
    from psxavenc_amd.mdec import query_geometry
    assert query_geometry(codec, w, h, cap).fits
    base = S.shared(("k313 long", codec, w, h), lambda: long_rows(codec, w, h, cap))
    K11.launch_twice(torch_cuda, codec, w, h, K.repeat(base, n, 7 * n + lanes), cap, lanes, False)
    K11.launch_twice(torch_cuda, codec, w, h, [base[1]] * n, cap, lanes, True)


# ---------------------------------------------------------------- a pass that only counts
@pytest.mark.parametrize("n", SHAPES)
def test_a_pass_that_only_counts(torch_cuda, n):
    """v2, 256x128: the frame made to fool this shape's judge (tests/test_gpu_mdec_sampled_count.py); its warm launch ends on a pass
    that only counts -- the count-only arm reads the doubled tile -- which the diagnostics instantiation's records have to show"""
    w, h = 256, 128
    large = S.shape_of(torch_cuda, n)
    r = S.shared(("fooled", w, h, large), lambda: S.fooled_row(w, h, large))
    for uniform_budget in (True, False):
        K11.launch_twice(torch_cuda, 0, w, h, [r] * n, S.CAP, 2, uniform_budget)
    env = {"PSXHIP_MDEC_STATS": "1", "PSXHIP_MDEC_TRUST": "1"}
    rec = K11.launch_twice(torch_cuda, 0, w, h, [r] * n, S.CAP, 1, True, env=env, want_records=True)
    _, _, counting, passes = K11.pass_facts(rec)
    print("%s: a pass that only counts on %d of %d, passes %s" % (r.name, (counting >= 1).sum(), n, np.bincount(passes).tolist()))
    assert (counting >= 1).sum() * 4 >= 3 * n
