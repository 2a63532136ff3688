#!/usr/bin/env python3
"""What the beam encoder ("psxhip ADPCM beam v1") gains and costs on an MI355X, beside the plain encoder: a
record, no thresholds.

  python tools/gpu_adpcm_beam_probe.py --out profiles/<beam kernel rev>_probe.json

Material: bench.py's `xacd` job shape (XA channels x stereo at 37800 Hz, 4-bit, the device's synth_pcm) on its tonal (kind 0), gated
(kind 5) and white (kind 2) signals, and the audio leg of one STR stream (one stereo XA channel, tonal).  Per material, for the plain
encoder (beam 0) and beam 1 .. 4 through the same session (psxhip_adpcm_session_set_beam): the speculate launch's and the verify
passes' milliseconds (psxhip_adpcm_session_set_timing: HIP events, median [min, max] over the repeats, the widths alternated inside
each repeat), the verify-pass count, the SNR of the records through the device decoder and psxhip_adpcm_sse_device (all chains
together and the worst chain), and the share of units whose record differs from the plain encoder's.  Needs the GPU: there is no
fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--audio-seconds", type=float, default=600.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--str-seconds", type=float, default=120.0)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "gpu_adpcm_beam_probe needs an MI355X"
    from psxavenc_amd import adpcm, adpcm_decode, synth

    dev = torch.device("cuda:0")
    L = adpcm._bind()
    L.psxhip_adpcm_kernel_rev.restype = ctypes.c_char_p
    L.psxhip_adpcm_beam_kernel_rev.restype = ctypes.c_char_p
    settings = adpcm.XaSettings(adpcm.PSX_AUDIO_XA_FORMAT_XACD, True, 37800, 4, 1, 0)
    sps = adpcm.xa_get_samples_per_sector(settings)
    record = {"kernel_rev": L.psxhip_adpcm_beam_kernel_rev().decode(), "plain_kernel_rev": L.psxhip_adpcm_kernel_rev().decode(),
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "method": "one session per material; per repeat every width in turn: reset, set_beam, run with timing (HIP events round the "
                        "speculate launch and round the verify passes); milliseconds are median [min, max]; SNR = 10 log10(sum x^2 / sum (y - x)^2) "
                        "of the device decoder's output against the input, from psxhip_adpcm_sse_device's sums; beam 0 is the plain encoder",
              "materials": {}}
    legs = [("xacd tonal (synth kind 0)", args.channels, args.audio_seconds, 0), ("xacd gated (synth kind 5)", args.channels, args.audio_seconds, 5),
            ("xacd white (synth kind 2)", args.channels, args.audio_seconds, 2), ("one STR stream's audio, tonal (synth kind 0)", 1, args.str_seconds, 0)]
    for label, n_ch, seconds, kind in legs:
        n_sectors = int(seconds * 37800 / sps)
        n_frames, units_per_chain = n_sectors * sps, n_sectors * 72
        total_units = 2 * n_ch * units_per_chain
        chains = adpcm.make_chains([c * n_frames * 2 + side for c in range(n_ch) for side in range(2)], 2, n_frames, units_per_chain, unit_stride=2)
        base = np.array([c * n_sectors * 144 + side for c in range(n_ch) for side in range(2)], np.int32)
        pcm = torch.empty((n_ch, n_frames * 2), dtype=torch.int16, device=dev)
        for c in range(n_ch):
            for side in range(2):
                synth.pcm_device(1, 2 * c + side, 0, n_frames, kind, device=0, out=pcm[c][side:], pitch=2)
        d_units = torch.zeros((n_ch * n_sectors * 144, 16), dtype=torch.uint8, device=dev)
        d_out = torch.zeros_like(pcm).reshape(-1)
        chunk, warm = adpcm.pick_chunking(total_units, rows=4)
        sess = adpcm.AdpcmSession(pcm.reshape(-1), chains, base, 4, 4, d_units=d_units, chunk_units=chunk, warmup_units=warm)
        sess.set_timing(True)
        init = np.zeros((2 * n_ch, 2), np.int32)
        ms = {b: {"speculate": [], "verify": []} for b in range(5)}
        passes, quality, plain_units = {}, {}, None
        for r in range(args.repeats + 1):                       # (the first round warms every shape up and takes the quality figures)
            for beam in range(5):
                sess.reset()
                sess.set_beam(beam)
                final, _ = sess.run(init)
                if r == 0:
                    passes[beam] = sess.passes
                    st = adpcm_decode.decode_chains_chunked(d_units, chains, base, 4, 4, d_out)[0]
                    assert np.array_equal(st.cpu().numpy(), final), "the decoder does not end where the encoder says it did"
                    _, sums = adpcm_decode.adpcm_sse(d_out, pcm.reshape(-1), chains)
                    s = sums.cpu().numpy().astype(np.float64)
                    per_chain = adpcm_decode.snr_db(sums.cpu().numpy())
                    if beam == 0:
                        plain_units = d_units.clone()
                    quality[beam] = {"snr_db": round(float(10 * np.log10(s[:, 1].sum() / max(s[:, 0].sum(), 1.0))), 3),
                                     "worst_chain_snr_db": round(float(min(per_chain)), 3),
                                     "share_of_units_that_differ_from_plain": round(float((d_units != plain_units).any(dim=1).float().mean()), 4)}
                else:
                    a, b = sess.last_timing()
                    ms[beam]["speculate"].append(a)
                    ms[beam]["verify"].append(b)
        out = {"job": "%d XA channel(s) x stereo x %.0f s @ 37800 Hz, 4-bit: %d chains of %d units" % (n_ch, seconds, 2 * n_ch, units_per_chain),
               "total_units": total_units, "chunk_units": chunk, "warmup_units": warm, "widths": {}}
        for beam in range(5):
            t = {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms[beam].items()}
            out["widths"]["beam %d%s" % (beam, " (plain encoder)" if beam == 0 else "")] = dict(
                quality[beam], milliseconds=t, verify_passes=passes[beam],
                units_per_s_speculate=round(total_units / (t["speculate"][0] * 1e-3)))
        record["materials"][label] = out
        sess.close()
        del pcm, d_units, d_out, plain_units
        torch.cuda.empty_cache()
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
