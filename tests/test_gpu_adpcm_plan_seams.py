"""Both sides of every seam the ADPCM host layer's plan (psxavenc_amd/csrc/adpcm_plan.cpp) routes by, on the device and against the
oracle: the per-call fast path and the batch path, serial chains and chains cut along time.  All routes give the same bytes, so
bytes cannot tell them apart -- which side a call takes is held by tests/test_adpcm_plan_cpu.py; here each side runs and is right."""
import numpy as np
import pytest

import adpcm_decode_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_units", [511, 512])
@pytest.mark.parametrize("n_streams", [1, 4, 5])
def test_spu_host_encode_on_both_sides(n_streams, n_units):
    """up to four streams may take the per-call path, five never; 512 units of at most eight chains are cut along time, 511 are not"""
    from psxavenc_amd import adpcm
    n = 28 * n_units - 5
    pcm = np.stack([O.synth_pcm(41, c, 100 * c, n, c % 6) for c in range(n_streams)])
    start = np.array([[3 * c, -2 * c] for c in range(n_streams)], np.int32)
    st = start.copy()
    out = adpcm.spu_encode_streams(pcm, states=st)
    assert out.shape == (n_streams, 16 * n_units)
    for c in range(n_streams):
        want, wst = O.spu_encode(pcm[c], state=O.Chan(int(start[c, 0]), int(start[c, 1])))
        assert np.array_equal(out[c], want), c
        assert st[c].tolist() == [wst.prev1, wst.prev2], c


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("n_streams,n_sectors", [(1, 2), (1, 3), (1, 6), (1, 7), (2, 1)])
def test_xa_host_encode_on_both_sides(n_streams, n_sectors, bits):
    """one stream of up to six sectors may take the per-call path while its samples fit the staging limit (two 4-bit sectors do, three
    do not); seven sectors, or two streams, take the batch"""
    from psxavenc_amd import adpcm
    s, os_ = adpcm.XaSettings(1, 1, 37800, bits, 1, 2), O.XaSettings(1, 1, 37800, bits, 1, 2)
    sps = adpcm.xa_get_samples_per_sector(s)            # per channel
    n = sps * n_sectors - 9
    pcm = np.zeros((n_streams, 2 * (n + 4032)), np.int16)           # (the oracle reads a sector's worth past the end)
    for i in range(n_streams):
        pcm[i, 0:2 * n:2] = O.synth_pcm(43, 2 * i, 0, n, i)
        pcm[i, 1:2 * n:2] = O.synth_pcm(43, 2 * i + 1, 0, n, 5)
    st = np.zeros((n_streams, 2, 2), np.int32)
    lbas = [150 + 10 * i for i in range(n_streams)]
    out = adpcm.xa_encode_streams(s, pcm[:, :2 * n], n, lbas=lbas, states=st)
    assert out.shape == (n_streams, 2352 * n_sectors)
    for i in range(n_streams):
        want, wst = O.xa_encode(os_, pcm[i], n, lba=lbas[i])
        assert np.array_equal(out[i], want), i
        assert st[i].tolist() == [[wst.left.prev1, wst.left.prev2], [wst.right.prev1, wst.right.prev2]], i


@pytest.mark.parametrize("n_units", [511, 512])
def test_spu_host_decode_on_both_sides(n_units):
    """one stream of 512 blocks is decoded in chunks, of 511 serially"""
    from psxavenc_amd import spu_decode_streams
    blocks, _ = O.spu_encode(O.synth_pcm(47, 0, 0, 28 * n_units, 2))
    want, want_state, _ = R.decode_chain(blocks.reshape(-1, 16), 4, 5, (11, -7))
    st = np.array([[11, -7]], np.int32)
    got = spu_decode_streams(blocks.reshape(1, -1), st)
    assert np.array_equal(got[0], want) and tuple(st[0]) == tuple(want_state)


@pytest.mark.parametrize("n_sectors", [3, 4])
def test_xa_host_decode_on_both_sides(n_sectors):
    """a mono 4-bit sector holds 144 units: three sectors stay below the 512 units of the threshold, four pass it"""
    from psxavenc_amd import adpcm, xa_decode_streams
    s = adpcm.XaSettings(0, 0, 37800, 4, 1, 0)
    n = adpcm.xa_get_samples_per_sector(s) * n_sectors
    sectors = adpcm.xa_encode_streams(s, O.synth_pcm(53, 0, 0, n, 0).reshape(1, -1), n)
    st = np.zeros((1, 2, 2), np.int32)
    got, status = xa_decode_streams(s, sectors, st)
    want, wst = R.decode_xa(sectors[0], 2336, 4, 0)
    assert status.tolist() == [[0] * n_sectors] and np.array_equal(got[0], want) and st[0, :1].tolist() == [list(x) for x in wst]
