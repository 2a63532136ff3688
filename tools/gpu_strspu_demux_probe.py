#!/usr/bin/env python3
"""Times the STRSPU reader (psxhip_strspu_demux_device) on 44100 Hz stereo at 2x: 1000 frames of 320x240 at 15 fps, muxed on the
device (10 000 sectors, 1667 of them audio), one stream and eight.

  python tools/gpu_strspu_demux_probe.py --out profiles/<kernel rev>_probe.json

Legs, by the method of tools/gpu_adpcm_decode_probe.py: the new demux; the existing format 9 demux over the same bytes (what a caller
had before: the audio chunks counted as `other`); a device-to-device copy of the same bytes (what moving the stream once costs).
Device events around every leg, every shape warmed up first, the legs alternated inside each repeat, median [min, max] over the
repeats.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1000, help="calls inside one timed leg: a window of tenths of a second")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "gpu_strspu_demux_probe needs an MI355X"
    from psxavenc_amd import strdemux, strmux, synth

    dev = torch.device("cuda:0")
    W, H = 320, 240
    s = strmux.settings(fmt=strmux.FORMAT_STRSPU, codec=0, width=W, height=H, fps_num=15, cd_speed=2, channels=2, frequency=44100,
                        tail=strmux.TAIL_COMPLETE)
    s9 = strmux.settings(fmt=9, codec=0, width=W, height=H, fps_num=15, cd_speed=2, channels=0)
    pl = strmux.plan(s, args.frames)
    n_pcm = (pl.n_audio_sectors + 1) * pl.audio_samples_per_sector
    record = {"kernel_rev": strdemux.strspu_demux_kernel_rev(), "str_demux_kernel_rev": strdemux.kernel_rev(),
              "device": torch.cuda.get_device_name(0),
              "job": "%d frames of %dx%d at 15 fps, 44100 Hz stereo, 2x: %d sectors, %d audio" % (args.frames, W, H, pl.n_sectors, pl.n_audio_sectors),
              "repeats": args.repeats, "calls_per_leg": args.calls,
              "method": "HIP events around %d back-to-back calls per leg; milliseconds per call, median [min, max] over the repeats, legs "
                        "alternated" % args.calls, "streams": {}}
    reader = strdemux.StrReader(0)
    mux = strmux.StrMuxer((0,))
    for S in (1, 8):
        d_frames = torch.stack([synth.frames_device(W, H, 1 + i, 0, args.frames, 6, device=0) for i in range(S)])
        d_pcm = torch.zeros((S, n_pcm * 2), dtype=torch.int16, device=dev)
        for i in range(S):
            for side in range(2):
                synth.pcm_device(1 + i, side, 0, n_pcm, 0, device=0, out=d_pcm[i][side:], pitch=2)
        d_sectors, p = mux.encode_device(s, d_frames, d_pcm)
        del d_frames, d_pcm
        n, K, stride = p.n_sectors, p.n_audio_sectors, p.max_frame_size
        kw = dict(d_bs=torch.zeros((S, args.frames, stride), dtype=torch.uint8, device=dev),
                  d_sizes=torch.zeros((S, args.frames), dtype=torch.int32, device=dev),
                  d_info=torch.zeros((S, args.frames, 8), dtype=torch.int32, device=dev),
                  d_summary=torch.zeros((S, 8), dtype=torch.int32, device=dev), table=False)
        d_units = torch.zeros((S, K * 126, 16), dtype=torch.uint8, device=dev)
        d_chunk = torch.zeros((S, K, 8), dtype=torch.int32, device=dev)
        d_asum = torch.zeros((S, 4), dtype=torch.int32, device=dev)
        d_none = torch.zeros((S, 0, 2048), dtype=torch.uint8, device=dev)
        d_copy = torch.empty_like(d_sectors)

        def new():
            return reader.demux_strspu_device(s, d_sectors, args.frames, stride, first_frame=1, audio_capacity=K, d_units=d_units,
                                              d_chunk_info=d_chunk, d_audio_summary=d_asum, **kw)

        def old():
            return reader.demux_device(s9, d_sectors, args.frames, stride, first_frame=1, xa_capacity=0, d_xa=d_none, **kw)

        def copy():
            return d_copy.copy_(d_sectors)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.calls

        # warm up every shape; the answers are sane before anything is timed
        new(), old(), copy()
        torch.cuda.synchronize()
        out = new()
        torch.cuda.synchronize()
        assert (out["summary"][:, 1].cpu().numpy() == K).all() and (out["summary"][:, 5].cpu().numpy() == args.frames).all()
        assert (d_asum.cpu().numpy()[:, :2] == K).all() and not d_chunk[:, :, 1].any()
        t = {"strspu demux": [], "format 9 demux": [], "device copy": []}
        for _ in range(args.repeats):
            t["strspu demux"].append(timed(new))
            t["format 9 demux"].append(timed(old))
            t["device copy"].append(timed(copy))
        ms = {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
        record["streams"][str(S)] = {
            "sectors": S * n, "audio_sectors": S * K, "milliseconds_per_call": ms,
            "sectors_per_s": {k: round(S * n / (v[0] * 1e-3)) for k, v in ms.items()},
            "bytes_per_s_in": {k: round(S * n * 2048 / (v[0] * 1e-3)) for k, v in ms.items()},
            "audio_half_ms": round(ms["strspu demux"][0] - ms["format 9 demux"][0], 4),
        }
        del d_sectors, d_units, d_copy, kw
        torch.cuda.empty_cache()
    mux.close()
    reader.close()
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
