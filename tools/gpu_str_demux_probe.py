#!/usr/bin/env python3
"""Times the STR reader's demux (psxhip_str_demux_device) on config 3's stream -- strcd, 1000 frames of 320x240 at 15 fps, stereo 37800 Hz
4-bit XA -- resident in HBM, for S = 1 and S = 8 streams per call, beside a device-to-device copy of the same stream bytes
(tensor.copy_: a demux reads each byte once and writes it once, as the copy does) and beside psxhip_str_encode_device's own time for
the stream.

  python tools/gpu_str_demux_probe.py --out profiles/<kernel rev>_probe.json

Device events around every leg, every shape warmed up first, the legs alternated inside each repeat, median [min, max] over the
repeats.  Needs the GPU: there is no fallback.  The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats
-- python tools/gpu_str_demux_probe.py --repeats 1` (tracing slows the host; its numbers are not mixed with these)."""
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
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "gpu_str_demux_probe needs an MI355X"
    from psxavenc_amd import strdemux, strmux, synth

    dev = torch.device("cuda:0")
    w, h = 320, 240
    s = strmux.settings()
    pl = strmux.plan(s, args.frames)
    n_pcm = pl.audio_samples_per_sector * (pl.n_audio_sectors + 2)
    stride = pl.max_frame_size
    record = {"kernel_rev": strdemux.kernel_rev(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "job": "strcd, %d frames of %dx%d @ 15 fps, stereo 37800 Hz 4-bit XA: %d sectors per stream" % (args.frames, w, h, pl.n_sectors),
              "method": "HIP events around each leg; median [min, max] milliseconds over the repeats, legs alternated in one process",
              "streams": {}}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    reader = strdemux.StrReader(0)
    for S in args.streams:
        d_frames = torch.stack([synth.frames_device(w, h, 1 + i, 0, args.frames, 4) for i in range(S)])
        d_pcm = torch.zeros((S, n_pcm * 2), dtype=torch.int16, device=dev)
        for i in range(S):
            for side in range(2):
                synth.pcm_device(1 + i, side, 0, n_pcm, 0, device=0, out=d_pcm[i][side:], pitch=2)
        mux = strmux.StrMuxer((0,))
        d_sectors, p = mux.encode_device(s, d_frames, d_pcm)
        nf = p.n_frames_encoded
        d_copy = torch.empty_like(d_sectors)
        out = reader.demux_device(s, d_sectors, nf, stride, first_frame=1)

        def demux():
            return reader.demux_device(s, d_sectors, nf, stride, first_frame=1, d_bs=out["bs"], d_sizes=out["sizes"], d_info=out["info"],
                                       d_xa=out["xa"], d_table=out["table"], d_summary=out["summary"])

        # warm up every shape; the answer is a whole stream before anything is timed
        demux()
        d_copy.copy_(d_sectors)
        mux.encode_device(s, d_frames, d_pcm, d_out=d_copy)
        torch.cuda.synchronize()
        summary = out["summary"].cpu().numpy()
        assert (summary[:, 5] == nf).all() and not out["info"][:, :, 7].any().item() and torch.equal(d_copy, d_sectors)
        t = {"demux": [], "copy": [], "encode": []}
        for _ in range(args.repeats):
            t["demux"].append(timed(demux)[0])
            t["copy"].append(timed(lambda: d_copy.copy_(d_sectors))[0])
            t["encode"].append(timed(lambda: mux.encode_device(s, d_frames, d_pcm, d_out=d_copy))[0])
        ms = {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
        nbytes = d_sectors.numel()
        record["streams"][str(S)] = {
            "stream_bytes": nbytes, "frames_per_stream": nf, "milliseconds": ms,
            "demux_over_copy": round(ms["demux"][0] / ms["copy"][0], 3), "demux_over_encode": round(ms["demux"][0] / ms["encode"][0], 4),
            "demux_bytes_per_s_read_plus_written": round(2 * nbytes / (ms["demux"][0] * 1e-3)),
            "copy_bytes_per_s_read_plus_written": round(2 * nbytes / (ms["copy"][0] * 1e-3))}
        mux.close()
        del d_frames, d_pcm, d_sectors, d_copy, out
        torch.cuda.empty_cache()
    reader.close()
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
