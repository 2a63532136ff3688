#!/usr/bin/env python3
"""Times the ADPCM decoder's kernels beside the encoder's speculate kernel on config 5's job (8 XA channels x stereo x 60 minutes at
37800 Hz, 4-bit: 16 chains of 4.86 M sound units), on tonal (kind 0) and white (kind 2) material from the device's synth_pcm.

  python tools/gpu_adpcm_decode_probe.py --out profiles/<kernel rev>_probe.json

Legs: the encoder's speculate launch and verify passes (psxhip_adpcm_session_set_timing), the decoder's chunked call with its
speculate launch and verify passes apart (psxhip_adpcm_decode_set_timing), the serial-per-chain decode, the squared-error kernel, the
sector disassembly.  Device events around every leg, every shape warmed up first, the legs alternated inside each repeat, median
[min, max] over the repeats.  Bytes per second count the algorithmic bytes: a 4-bit unit is 16 bytes in and 56 out.  Needs the GPU:
there is no fallback.  Kernel-level attribution comes from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/gpu_adpcm_decode_probe.py --repeats 1` (tracing slows the host; its numbers are not mixed with these)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--audio-seconds", type=float, default=3600.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--serial-repeats", type=int, default=2, help="the serial-per-chain decode takes seconds: fewer repeats")
    ap.add_argument("--chunk-units", type=int, default=0, help="decoder chunk length (0: the library's choice)")
    args = ap.parse_args()

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "gpu_adpcm_decode_probe needs an MI355X"
    from psxavenc_amd import adpcm, adpcm_decode, synth

    dev = torch.device("cuda:0")
    settings = adpcm.XaSettings(adpcm.PSX_AUDIO_XA_FORMAT_XACD, True, 37800, 4, 1, 0)
    sps = adpcm.xa_get_samples_per_sector(settings)
    n_sectors = int(args.audio_seconds * 37800 / sps)
    n_ch = args.channels
    n_frames = n_sectors * sps
    units_per_chain = n_sectors * 72
    total_units = 2 * n_ch * units_per_chain
    chains = adpcm.make_chains([c * n_frames * 2 + side for c in range(n_ch) for side in range(2)], 2, n_frames, units_per_chain, unit_stride=2)
    base = np.array([c * n_sectors * 144 + side for c in range(n_ch) for side in range(2)], np.int32)
    import ctypes
    L = adpcm._bind()
    L.psxhip_adpcm_kernel_rev.restype = ctypes.c_char_p
    record = {"kernel_rev": adpcm_decode.kernel_rev(), "encoder_kernel_rev": L.psxhip_adpcm_kernel_rev().decode(),
              "device": torch.cuda.get_device_name(0), "job": "%d XA channels x stereo x %.0f s @ 37800 Hz, 4-bit: %d chains of %d units"
              % (n_ch, args.audio_seconds, 2 * n_ch, units_per_chain), "total_units": total_units, "sectors": n_ch * n_sectors,
              "bytes_per_unit": {"in": 16, "out": 56}, "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": args.repeats,
              "method": "HIP events around each leg; median [min, max] milliseconds over the repeats, legs alternated", "content": {}}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    for label, kind in (("tonal (synth kind 0: two tones + noise)", 0), ("white (synth kind 2: full-scale noise)", 2)):
        pcm = torch.empty((n_ch, n_frames * 2), dtype=torch.int16, device=dev)
        for c in range(n_ch):
            for side in range(2):
                synth.pcm_device(1, 2 * c + side, 0, n_frames, kind, device=0, out=pcm[c][side:], pitch=2)
        d_units = torch.zeros((n_ch * n_sectors * 144, 16), dtype=torch.uint8, device=dev)
        enc_chunk, enc_warm = adpcm.pick_chunking(total_units)
        sess = adpcm.AdpcmSession(pcm.reshape(-1), chains, base, 4, 4, d_units=d_units, chunk_units=enc_chunk, warmup_units=enc_warm)
        sess.set_timing(True)
        init = np.zeros((2 * n_ch, 2), np.int32)
        enc_final, _ = sess.run(init)
        d_out = torch.zeros_like(pcm).reshape(-1)
        d_sectors = torch.cat([adpcm.xa_assemble_device(d_units[c * n_sectors * 144:], n_sectors, settings) for c in range(n_ch)])
        d_back = torch.zeros_like(d_units)
        adpcm_decode.set_timing(True)

        def chunked():
            st, passes = adpcm_decode.decode_chains_chunked(d_units, chains, base, 4, 4, d_out, chunk_units=args.chunk_units)
            return st, passes

        def serial():
            return adpcm_decode.decode_chains_device(d_units, chains, base, 4, 4, d_out)

        # warm up every shape; the answers agree before anything is timed
        st_c, passes = chunked()
        assert np.array_equal(st_c.cpu().numpy(), enc_final), "the chunked decode's final states are not the encoder's"
        chunked_pcm = d_out.clone()
        st_s = serial()
        assert np.array_equal(st_s.cpu().numpy(), enc_final) and torch.equal(chunked_pcm, d_out), "serial and chunked decode differ"
        del chunked_pcm
        adpcm_decode.adpcm_sse(d_out, pcm.reshape(-1), chains)
        _, d_status = adpcm_decode.xa_disassemble(d_sectors, settings, d_units=d_back)
        torch.cuda.synchronize()
        assert torch.equal(d_back, d_units) and not d_status.any()

        t = {k: [] for k in ("encode speculate", "encode verify", "decode chunked (whole call)", "decode speculate", "decode verify",
                             "decode serial per chain", "sse", "disassemble")}
        passes_seen = {"encode": [], "decode": []}
        for r in range(args.repeats):
            sess.reset()
            _, _ = sess.run(init)
            a, b = sess.last_timing()
            t["encode speculate"].append(a)
            t["encode verify"].append(b)
            passes_seen["encode"].append(sess.passes)
            ms, (_, p) = timed(chunked)
            a, b = adpcm_decode.last_timing()
            t["decode chunked (whole call)"].append(ms)
            t["decode speculate"].append(a)
            t["decode verify"].append(b)
            passes_seen["decode"].append(p)
            if r < args.serial_repeats:
                t["decode serial per chain"].append(timed(serial)[0])
            t["sse"].append(timed(lambda: adpcm_decode.adpcm_sse(d_out, pcm.reshape(-1), chains))[0])
            t["disassemble"].append(timed(lambda: adpcm_decode.xa_disassemble(d_sectors, settings, d_units=d_back))[0])
        ms = {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in t.items()}
        moved = {"decode speculate": 72, "decode chunked (whole call)": 72, "decode serial per chain": 72, "sse": 112,
                 "disassemble": 2352 / 144 + 16, "encode speculate": 72}
        rates = {}
        for k, per_unit in moved.items():
            bps = total_units * per_unit / (ms[k][0] * 1e-3)
            rates[k] = {"units_per_s": round(total_units / (ms[k][0] * 1e-3)), "bytes_per_s": round(bps), "share_of_hbm_peak": round(bps / HBM_PEAK, 4)}
        _, sums = adpcm_decode.adpcm_sse(d_out, pcm.reshape(-1), chains)
        record["content"][label] = {
            "milliseconds": ms, "rates": rates, "verify_passes": passes_seen,
            "decoder_chunking": {"chunk_units": args.chunk_units or "library", "warmup_units": 64},
            "encoder_chunking": {"chunk_units": enc_chunk, "warmup_units": enc_warm},
            "decode_speculate_over_encode_speculate": round(ms["decode speculate"][0] / ms["encode speculate"][0], 4),
            "snr_db_per_chain": [round(float(x), 2) for x in adpcm_decode.snr_db(sums.cpu().numpy())],
        }
        sess.close()
        del pcm, d_units, d_out, d_sectors, d_back
        torch.cuda.empty_cache()
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
