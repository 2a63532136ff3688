"""The front ends' plans (picture_plan.cpp, resample_plan.cpp) against the device they plan for: the two drivers of the CPU tests,
built with plain g++, are asked what the plans decide for THIS device's LDS size and CU count, and both sides of every seam they
name are then run through the library, bit-exact against oracle/frontend_oracle.c and tests/resample_ref.py.

Scaler: the tile shapes either side of the plan's natural choice, and n_frames either side of the points where the number of vertical
segments changes.  Resampler: a design whose table the plan puts in LDS and one it leaves in memory, one and eight output channels, a
stream given as three calls whose lengths sit around H (the filter's half length, where the first outputs appear)."""
import numpy as np
import pytest

import oracle_lib as O
import resample_ref as R
import test_picture_plan_cpu as PP
import test_resample_plan_cpu as RP

pytestmark = pytest.mark.gpu

SCALER_GEOMETRIES = [(0, 200, 150, True, 128, 64), (1, 352, 288, False, 128, 64)]


@pytest.fixture(scope="module")
def device():
    """(LDS bytes per CU, CUs) as the Python mirrors report them"""
    import torch
    from psxavenc_amd import mdec
    return int(mdec.query_geometry(0, 320, 240, 9000).lds_bytes_per_cu), int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def picture_driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("picture_plan_seams"))
    exe = PP.build_driver(tmp, [])
    return lambda calls: PP.run_driver(exe, tmp, calls)


@pytest.fixture(scope="module")
def resample_driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("resample_plan_seams"))
    exe = RP.build_driver(tmp, [])
    return lambda calls: RP.run_driver(exe, tmp, calls)


def _pictures(geometry, n):
    """n pictures (eight distinct ones, repeated: frames are independent) and the oracle's frames"""
    fmt, sw, sh, full, dw, dh = geometry
    rng = np.random.default_rng(sw + dh)
    nbytes = sw * sh * 3 if fmt == 0 else sw * sh * 3 // 2
    base = rng.integers(0, 256, (8, nbytes), dtype=np.uint8)
    base[1] = 255
    base[2] = 0
    base[3, ::2] = 255
    want = O.scaler_convert(fmt, sw, sh, full, dw, dh, base)
    idx = np.arange(n) % 8
    return base[idx], want[idx]


@pytest.mark.parametrize("geometry", SCALER_GEOMETRIES, ids=["rgb", "yuv"])
def test_scaler_tiles_and_segments_either_side_of_the_plan_s_choices(geometry, device, picture_driver, monkeypatch):
    import torch
    from psxavenc_amd.frontend import Scaler
    fmt, sw, sh, full, dw, dh = geometry
    lds, n_cu = device
    monkeypatch.delenv("PSXHIP_SCALER_TILE", raising=False)
    monkeypatch.delenv("PSXHIP_SCALER_VSEGS", raising=False)
    k, got, blob = picture_driver([PP.tile_call(geometry, device, f) for f in (-1, 0, 1, 2, 3)])
    assert got[0][0] == 0, got[0]
    natural = PP.Tile(got[0][1], blob)
    at = k.shapes.index((natural.TW, natural.TH))
    assert natural.lds_bytes * 2 <= lds or at == 3
    pics, want = _pictures(geometry, 8)
    for forced in sorted({max(at - 1, 0), at, min(at + 1, 3)}):
        rc, text = got[1 + forced]
        assert rc == 0, (forced, text)                   # targets this small fit every shape: a refusal is a failure
        monkeypatch.setenv("PSXHIP_SCALER_TILE", str(forced))
        sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
        monkeypatch.delenv("PSXHIP_SCALER_TILE")
        assert np.array_equal(sc.convert_host(pics), want), "tile %d" % forced
        sc.close()
    # the segments, by the plan, for every n_frames up to where one segment is left: the natural tile either side of its last change
    # (a few hundred frames), the smallest tile either side of its first (a few frames)
    small = PP.Tile(got[1 + 3][1], blob)
    for tile, forced, pick in ((natural, None, -1), (small, "3", 0)):
        last = 4 * n_cu // tile.tiles_x + 2
        _, answers, _ = picture_driver([("vsegs", [n_cu, tile.tiles_x, tile.tiles_y, n, -1]) for n in range(1, last + 1)])
        vsegs = [PP.lists(text)[0][0] for _, text in answers]
        changes = [n for n in range(2, last + 1) if vsegs[n - 1] != vsegs[n - 2]]
        assert vsegs[0] == tile.tiles_y and vsegs[-1] == 1 and changes, (vsegs[0], vsegs[-1], changes)
        if forced:
            monkeypatch.setenv("PSXHIP_SCALER_TILE", forced)
        sc = Scaler(fmt, sw, sh, dw, dh, src_full_range=full)
        monkeypatch.delenv("PSXHIP_SCALER_TILE", raising=False)
        for n in (changes[pick] - 1, changes[pick]):
            pics, want = _pictures(geometry, n)
            got_frames = sc.convert_device(torch.from_numpy(pics).to("cuda:0")).cpu().numpy()
            assert np.array_equal(got_frames, want), "tile %dx%d, n_frames %d (%d segments by the plan)" % (tile.TW, tile.TH, n, vsegs[n - 1])
        sc.close()


def test_resampler_table_in_lds_or_not_one_and_eight_channels_calls_around_h(device, resample_driver):
    import torch
    from psxavenc_amd import resample as rs
    lds, n_cu = device
    designs = [(48000, 37800), (44100, 44099)]
    cases = [(s, d, ch) for s, d in designs for ch in (1, 8)]
    _, got, _ = resample_driver([("shape", [s, d, ch, lds, n_cu]) for s, d, ch in cases])
    shapes = [RP.lists(text)[0] for rc, text in got if rc == 0]
    assert len(shapes) == len(cases) and [s[1] for s in shapes] == [1, 1, 0, 0], shapes          # the plan: the first table in LDS, the second not
    for (src, dst, ch), (span, coef_lds, lds_bytes, grid_max) in zip(cases, shapes):
        L, M_, P, T, H, _ = R.params(src, dst)
        assert lds_bytes <= lds and grid_max >= n_cu
        n = 3000 + 2 * 256 * M_ // L
        rng = np.random.default_rng(src + ch)
        x = rng.integers(-32768, 32768, (n, ch), dtype=np.int16)
        x[:4] = 32767
        x[4:8] = -32768
        _, _, coef = rs.design(src, dst)
        want = R.statement(0, [x.reshape(-1)], ch, src, dst, rs.default_matrix(ch, ch), coef, flush=True)
        for first, second in ((H - 1, 2), (H, 1), (H + 1, H - 1)):
            r = rs.Resampler(0, ch, src, ch, dst)
            cuts = [0, first, first + second, n]
            outs = [r.convert_device(torch.from_numpy(x[a:b].copy()).to("cuda:0"), flush=b == n).cpu().numpy() for a, b in zip(cuts, cuts[1:])]
            r.close()
            assert len(outs[0]) == RP.outputs_of(src, dst, 0, first, 0)
            assert np.array_equal(np.concatenate(outs), want), (src, dst, ch, first, second)
