#!/usr/bin/env python3
"""Times the refinement (psxhip_mdec_refine_frames_device) beside the plain encode on the batch bench.py measures
(1000 x 320x240 v2, noise +-4, budget 8192) and on the scene-structured content (psxavenc_amd/mixed.py), and records what it does to
the frames: the shares refined, declined and untouched, and the mean PSNR change through the device decoder and psxhip_mdec_sse_device.

  python tools/gpu_mdec_shed_probe.py --out profiles/mdec-shed-k1.0_probe.json

Device events around windows of back-to-back launches, every leg warmed up first, the legs alternated inside one run, median and
spread over the windows reported.  A refine launch needs rows and results as the plain encode left them, so its leg is encode + refine
and the refinement's own time is the difference to the encode leg of the same window.  Sets no thresholds.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0, help="target length of a timed window")
    args = ap.parse_args()

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "gpu_mdec_shed_probe needs an MI355X"
    from psxavenc_amd import MdecDecoder, decode, mixed, synth
    from psxavenc_amd.mdec import MdecEncoder, refine_records, shed_kernel_rev

    w, h, budget, n = 320, 240, 8192, args.frames
    record = {"kernel_rev": shed_kernel_rev(), "device": torch.cuda.get_device_name(0), "width": w, "height": h, "codec": "v2",
              "frames": n, "budget": budget, "windows": args.windows, "method": "HIP events around windows of back-to-back launches; "
              "median [min, max] microseconds per launch of the whole batch; refine = (encode + refine) - encode of the same window",
              "content": {}}
    for name, d_frames in (("noise +-4 (the bench.py batch)", synth.frames_device(w, h, 1, 0, n, 4, device=0)),
                           ("scene-structured (psxavenc_amd/mixed.py)", mixed.frames_device(w, h, 1, 0, n, device=0))):
        enc = MdecEncoder(0, w, h, max_frame_size=budget, device=0)
        dec = MdecDecoder(w, h)
        d_out, d_res = enc.encode_frames_device(d_frames, budget)
        _, d_px0, _ = dec.decode_frames_device(d_out, budget, levels=False)
        sse0 = decode.sse_device(d_px0, d_frames, w, h).cpu().numpy()
        res0 = d_res.cpu().numpy()
        content = {}
        for K in (1, 2, 3):
            enc.encode_frames_device(d_frames, budget, d_out=d_out, d_results=d_res)
            d_rec = enc.refine_frames_device(d_frames, budget, d_out, d_res, max_magnitude=K)
            _, d_px, d_dec = dec.decode_frames_device(d_out, budget, levels=False)
            sse = decode.sse_device(d_px, d_frames, w, h).cpu().numpy()
            torch.cuda.synchronize()
            assert (d_dec[:, 0] == 0).all()
            rec = refine_records(d_rec.cpu().numpy())
            refined = rec[:, 0] != 0
            eligible = (res0[:, 0] > 1) & (res0[:, 0] < 64)
            psnr0, psnr1 = decode.psnr(sse0, w, h), decode.psnr(sse, w, h)
            with np.errstate(invalid="ignore"):
                gain = np.where(sse == sse0, 0.0, psnr1 - psnr0)          # (a flat plane is exact either way: inf - inf)
            content["K=%d" % K] = {
                "share_refined": round(float(refined.mean()), 4), "share_declined": round(float((eligible & ~refined).mean()), 4),
                "share_untouched": round(float((~eligible).mean()), 4),
                "share_declined_nothing_fits": round(float((eligible & ~refined & (rec[:, 2] == 0)).mean()), 4),
                "mean_psnr_change_db_y_cb_cr_all_frames": [round(float(x), 4) for x in gain.mean(axis=0)],
                "mean_psnr_change_db_y_cb_cr_refined_frames": [round(float(x), 4) for x in gain[refined].mean(axis=0)] if refined.any() else None,
                "refined_frames_with_lower_luma_psnr": int((gain[refined, 0] < 0).sum()),
                "mean_bytes_used": [round(float(res0[:, 1].mean()), 1), round(float(d_res.cpu().numpy()[:, 1].mean()), 1)],
                "mean_levels_shed_per_refined_frame": round(float(rec[refined, 1].mean()), 1) if refined.any() else None,
            }

        def both(K):
            enc.encode_frames_device(d_frames, budget, d_out=d_out, d_results=d_res)
            enc.refine_frames_device(d_frames, budget, d_out, d_res, max_magnitude=K, d_refine=d_rec)

        legs = {"encode": lambda: enc.encode_frames_device(d_frames, budget, d_out=d_out, d_results=d_res),
                "encode + refine K=1": lambda: both(1), "encode + refine K=3": lambda: both(3)}
        reps = {}
        for leg, fn in legs.items():                       # warm up and size the window
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            reps[leg] = max(10, int(args.window_ms * 1e-3 / ((time.perf_counter() - t0) / 10)))
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
        for K in (1, 3):
            d = [x - y for x, y in zip(times["encode + refine K=%d" % K], times["encode"])]
            us["refine K=%d (difference per window)" % K] = [round(statistics.median(d), 2), round(min(d), 2), round(max(d), 2)]
        content["microseconds_per_launch"] = us
        content["launches_per_window"] = reps
        content["mean_quant_scale_plain"] = round(float(res0[:, 0].mean()), 3)
        record["content"][name] = content
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
