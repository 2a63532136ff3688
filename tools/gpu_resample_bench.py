"""Throughput of the audio front-end (psxhip_resampler_convert_device): 8 streams x 60 min of stereo 48 kHz
F32P in HBM -> 37.8 kHz interleaved S16 stereo, one handle and one call (with flush) per stream.  Prints one JSON line: the kernel
time from HIP events, the algorithmic GB/s and the fraction of the 8 TB/s HBM peak, and (--chain) the chained figure: the same
job resampled straight into the PCM buffer of config 5's XA path (xacd: 8 XA channels x stereo, 4-bit, speculate-and-verify
sessions, sector assembly) and encoded, against that XA path alone on the same buffer.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_resample_bench.py` for the kernel trace's figure."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import time  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from psxavenc_amd import resample  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chain", action="store_true", help="also time resample + the xacd XA path on the same job")
    args = ap.parse_args()
    src, dst = 48000, 37800
    n = int(src * args.seconds)
    d_in = [torch.rand((2, n), dtype=torch.float32, device="cuda:0") * 2 - 1 for _ in range(args.streams)]
    rs = [resample.Resampler(resample.PCM_F32P, 2, src, 2, dst) for _ in range(args.streams)]
    n_out = resample.output_count(src, dst, 0, n, True)
    # the outputs are the rows of one (streams, n_out * 2) buffer: the XA path's PCM in --chain
    pcm = torch.empty((args.streams, n_out * 2), dtype=torch.int16, device="cuda:0")
    d_out = [pcm[c].view(n_out, 2) for c in range(args.streams)]

    def step():
        for r, x, o in zip(rs, d_in, d_out):
            r.reset()
            r.convert_device(x, d_out=o, flush=True)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        for r in rs:
            r.reset()           # (synchronises: outside the timed region)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r, x, o in zip(rs, d_in, d_out):
            r.convert_device(x, d_out=o, flush=True)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    ms = min(times)
    read, written = args.streams * n * 2 * 4, args.streams * n_out * 2 * 2
    gbs = (read + written) / ms / 1e6
    row = {"tool": "gpu_resample_bench", "kernel_rev": resample.kernel_rev(),
           "workload": "%d x %.0f s stereo 48 kHz F32P -> 37.8 kHz S16 stereo" % (args.streams, args.seconds),
           "gb_read": round(read / 1e9, 3), "gb_written": round(written / 1e9, 3), "ms_min": round(ms, 4),
           "ms_median": round(sorted(times)[len(times) // 2], 4), "algorithmic_gbs": round(gbs, 1),
           "frac_of_8tbs": round(gbs / 8000, 4)}
    if args.chain:
        row.update(chain(args, rs, d_in, pcm, n_out))
    print(json.dumps(row), flush=True)


def chain(args, rs, d_in, pcm, n_out):
    """resample + config 5's XA path (bench.py bench_xacd at world size 1), and that XA path alone, on the same PCM buffer"""
    from psxavenc_amd import adpcm
    from psxavenc_amd.parallel import run_time_sharded
    settings = adpcm.XaSettings(adpcm.PSX_AUDIO_XA_FORMAT_XACD, True, 37800, 4, 1, 0)
    sps = adpcm.xa_get_samples_per_sector(settings)
    n_ch = args.streams
    n_sectors = n_out // sps
    chains = adpcm.make_chains([c * n_out * 2 + side for c in range(n_ch) for side in range(2)], 2, n_sectors * sps,
                               n_sectors * 72, unit_stride=2)
    base = np.array([c * n_sectors * 144 + side for c in range(n_ch) for side in range(2)], np.int32)
    d_units = torch.zeros((n_ch * n_sectors * 144, adpcm.record_bytes(4)), dtype=torch.uint8, device="cuda:0")
    init = np.zeros((2 * n_ch, 2), np.int32)
    chunk_units, warmup_units = adpcm.pick_chunking(int(chains["n_units"].sum()))
    sess = adpcm.AdpcmSession(pcm.reshape(-1), chains, base, 4, 4, d_units=d_units, lead_units=np.zeros(2 * n_ch, np.int32),
                              chunk_units=chunk_units, warmup_units=warmup_units)

    def xa():
        sess.reset()
        run_time_sharded(sess, 0, 1, None, init, device="cuda:0")
        return [adpcm.xa_assemble_device(d_units[c * n_sectors * 144:], n_sectors, settings, first_lba=0) for c in range(n_ch)]

    def timed(with_resample):
        best = None
        for i in range(args.warmup + args.steps):
            for r in rs:
                r.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if with_resample:
                for r, x, c in zip(rs, d_in, range(n_ch)):
                    r.convert_device(x, d_out=pcm[c].view(n_out, 2), flush=True)
            xa()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                best = dt if best is None else min(best, dt)
        return best

    xa_ms = timed(False)
    chain_ms = timed(True)
    return {"chain": "resample -> xacd XA path (%d channels x %d sectors, 4-bit, world size 1)" % (n_ch, n_sectors),
            "chain_ms_min": round(chain_ms, 3), "xa_only_ms_min": round(xa_ms, 3), "xa_sessions_passes": int(sess.passes)}


if __name__ == "__main__":
    main()
