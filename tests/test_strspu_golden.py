"""The audio lanes of format 8 against blocks recorded from the reference build's psx_audio_spu_encode
(tests/golden/strspu_ref.npz): the restatement the other tests check against (tests/strspu_ref.py over the oracle's SPU encoder, or
over the reference build where it is there) gives exactly these, so the format's audio is pinned where oracle/_ref is absent."""
import numpy as np

import oracle_lib as O
import strspu_ref as R


def test_restated_lanes_equal_the_recorded_reference_blocks():
    cases = R.golden_cases()
    assert len(cases) == 2
    for case, pcm, blocks in cases:
        ch, K, options = case["channels"], case["K"], case["options"]
        U = R.units_per_channel(K, ch, options)
        assert blocks.shape == (ch, U, 16) and U == K * (126 // ch) - (0 if options & R.NO_LEADING_DUMMY else 1)
        assert np.array_equal(R.lanes(pcm, ch, U), blocks), case
        # ... through the oracle's restatement in any case
        fitted = R.fit_pcm(pcm, ch, U)
        for c in range(ch):
            assert np.array_equal(O.spu_encode(fitted[c])[0].reshape(-1, 16), blocks[c]), (case, c)
    # one case is short of its fit (silence behind the PCM), the other longer (cut)
    assert [case["samples"] < 28 * R.units_per_channel(case["K"], case["channels"], case["options"]) for case, _, _ in cases] == [True, False]


def test_audio_sectors_of_the_recorded_lanes():
    """the chunks the restatement builds from them: header fields, dummy block, loop flag and trap block where the format puts them"""
    for case, pcm, blocks in R.golden_cases():
        ch, K, options = case["channels"], case["K"], case["options"]
        B, L = 126 // ch, 16 * (126 // ch)
        d = 0 if options & R.NO_LEADING_DUMMY else 1
        sec = R.audio_sectors(blocks, K, ch, 44100, options)
        assert sec.shape == (K, 2048)
        for k in range(K):
            hd = sec[k, :32]
            assert bytes(hd[:2]) == b"\x60\x01" and int(hd[2]) | int(hd[3]) << 8 == options & 0xFFFF
            assert [int(hd[8]), int(hd[12]) | int(hd[13]) << 8, int(hd[16]), int(hd[18]) | int(hd[19]) << 8] == [k + 1, 2016, ch, L]
            for c in range(ch):
                lane = sec[k, 0x20 + c * L: 0x20 + (c + 1) * L].reshape(B, 16)
                if k == 0 and d:
                    assert not lane[0].any()
                first = 1 if k == 0 and d else 0
                u0 = k * B + first - d
                assert np.array_equal(lane[first:B - 1], blocks[c][u0:u0 + B - 1 - first])
                if options & R.LOOP:
                    assert lane[B - 1, 1] == 3 and np.array_equal(np.delete(lane[B - 1], 1), np.delete(blocks[c][k * B + B - 1 - d], 1))
                elif k == K - 1:
                    assert lane[B - 1].tolist() == [0, 5] + [0] * 14
                else:
                    assert np.array_equal(lane[B - 1], blocks[c][k * B + B - 1 - d])
