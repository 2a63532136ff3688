#!/usr/bin/env python3
"""Times the decoder's kernels beside the encoder's on the batch bench.py measures (1000 x 320x240 v2, noise +-4, budget 8192) and on
the scene-structured content (psxavenc_amd/mixed.py), and beside the CPU oracle's reader on one core.

  python tools/gpu_decode_probe.py --out profiles/<kernel rev>_probe.json

Device events around windows of back-to-back launches (each window long enough that the clock's grain does not matter), every shape
warmed up first, the legs alternated inside one run, median and spread over the windows reported.  Needs the GPU: there is no
fallback.  Kernel-level attribution comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/gpu_decode_probe.py
--windows 1` (tracing slows the host; its numbers are not mixed with these)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0, help="target length of a timed window")
    ap.add_argument("--cpu-frames", type=int, default=200, help="frames the CPU oracle decodes for its rate")
    args = ap.parse_args()

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "gpu_decode_probe needs an MI355X"
    import oracle_lib as O
    from psxavenc_amd import MdecDecoder, decode, mixed, synth
    from psxavenc_amd.mdec import MdecEncoder

    w, h, budget, n = 320, 240, 8192, args.frames
    record = {"kernel_rev": decode.kernel_rev(), "device": torch.cuda.get_device_name(0), "width": w, "height": h, "codec": "v2",
              "frames": n, "budget": budget, "windows": args.windows, "method": "HIP events around windows of back-to-back launches; "
              "median [min, max] microseconds per launch of the whole batch", "content": {}}
    for name, d_frames in (("noise +-4 (the bench.py batch)", synth.frames_device(w, h, 1, 0, n, 4, device=0)),
                           ("scene-structured (psxavenc_amd/mixed.py)", mixed.frames_device(w, h, 1, 0, n, device=0))):
        enc = MdecEncoder(0, w, h, max_frame_size=budget, device=0)
        dec = MdecDecoder(w, h)
        d_out, d_res = enc.encode_frames_device(d_frames, budget)
        d_lv, d_px, d_dec = dec.decode_frames_device(d_out, budget)
        d_sse = decode.sse_device(d_px, d_frames, w, h)
        torch.cuda.synchronize()
        assert (d_dec[:, 0] == 0).all() and (d_res[:, 0] <= 63).all()
        legs = {
            "encode": lambda: enc.encode_frames_device(d_frames, budget, d_out=d_out, d_results=d_res),
            "parse (levels out)": lambda: dec.decode_frames_device(d_out, budget, frames=False, d_levels=d_lv, d_decoded=d_dec),
            "parse (verify only: no levels)": lambda: dec.decode_frames_device(d_out, budget, levels=False, frames=False, d_decoded=d_dec),
            "parse + reconstruct": lambda: dec.decode_frames_device(d_out, budget, d_levels=d_lv, d_frames=d_px, d_decoded=d_dec),
            "sse": lambda: decode.sse_device(d_px, d_frames, w, h, d_sse=d_sse),
        }
        reps = {}
        for leg, fn in legs.items():                       # warm up and size the window
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            per = (time.perf_counter() - t0) / 20
            reps[leg] = max(20, int(args.window_ms * 1e-3 / per))
        times = {leg: [] for leg in legs}
        for _ in range(args.windows):                      # the legs alternate: drift hits all of them alike
            for leg, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps[leg]):
                    fn()
                b.record()
                b.synchronize()
                times[leg].append(a.elapsed_time(b) * 1e3 / reps[leg])
        us = {leg: [round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)] for leg, t in times.items()}
        us["reconstruct (difference)"] = [round(us["parse + reconstruct"][0] - us["parse (levels out)"][0], 2)]
        # the CPU oracle's reader on one core, same rows
        rows = d_out[:args.cpu_frames].cpu().numpy()
        t0 = time.perf_counter()
        for i in range(rows.shape[0]):
            rc = O.mdec_decode(w, h, rows[i])[0]
            assert rc == 0
        cpu = (time.perf_counter() - t0) / rows.shape[0]
        res = d_res.cpu().numpy()
        sse = d_sse.cpu().numpy()
        record["content"][name] = {
            "microseconds_per_launch": us, "launches_per_window": reps,
            "frames_per_second": {leg: round(n / (v[0] * 1e-6), 1) for leg, v in us.items() if v[0] > 0},
            "parse_over_encode": round(us["parse (levels out)"][0] / us["encode"][0], 3),
            "cpu_oracle_decode_one_core": {"microseconds_per_frame": round(cpu * 1e6, 1), "frames_per_second": round(1 / cpu, 1),
                                           "frames": int(rows.shape[0])},
            "mean_quant_scale": round(float(res[:, 0].mean()), 3), "mean_bytes_used": round(float(res[:, 1].mean()), 1),
            "mean_psnr_db_y_cb_cr": [round(float(x), 2) for x in decode.psnr(sse, w, h).mean(axis=0)],
        }
        enc.close()
        dec.close()
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
