#!/usr/bin/env python3
"""Time psxhip_str_encode_device for format 8 (STRSPU: 44100 Hz stereo SPU-ADPCM, 2x) beside the STRCD call (37800 Hz 4-bit stereo
XA, 2x) over the same 1000 frames of 320x240 at 15 fps, on one build, in one process: `--streams` independent streams per call, frames
and PCM resident in HBM, sectors landing in HBM -- the protocol of bench.py's `strcd` config.  The two formats'
calls are timed in alternating rounds (host clock around calls that return when the sectors are complete); the video leg alone
(audio_channels 0) is timed beside them, so that one can see which leg bounds a call.  Prints one JSON line and writes it to --out.

    python tools/gpu_strspu_bench.py --streams 1 --out build/strspu_bench/strspu_bench_S1.json
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--amp", type=int, default=4)
    ap.add_argument("--audio-kind", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs an MI355X: a measurement path that finds no GPU fails"
    from psxavenc_amd import _lib, strmux, synth
    L = _lib.lib()
    L.psxhip_version.restype = L.psxhip_adpcm_kernel_rev.restype = __import__("ctypes").c_char_p
    w, h, n, S = 320, 240, args.frames, args.streams
    dev = "cuda:0"
    common = dict(codec=0, width=w, height=h, fps_num=15, fps_den=1, cd_speed=2)
    configs = {
        "strspu": strmux.settings(fmt=strmux.FORMAT_STRSPU, channels=2, frequency=44100, tail=strmux.TAIL_COMPLETE, **common),
        "strcd": strmux.settings(fmt=strmux.FORMAT_STRCD, **common),
        "strspu_video_only": strmux.settings(fmt=strmux.FORMAT_STRSPU, channels=0, tail=strmux.TAIL_COMPLETE, **common),
    }
    d_frames = torch.stack([synth.frames_device(w, h, args.seed + 17 * i, 0, n, args.amp, device=0) for i in range(S)])
    # a little more audio than either stream takes
    per_ch = max((strmux.plan(s, n).n_audio_sectors + 2) * max(strmux.plan(s, n).audio_samples_per_sector, 1) + 100 for s in configs.values())
    d_pcm = torch.zeros((S, per_ch * 2), dtype=torch.int16, device=dev)
    for i in range(S):
        for c in range(2):
            synth.pcm_device(args.seed, 2 * i + c, 0, per_ch, args.audio_kind, device=0, out=d_pcm[i][c:], pitch=2)
    state = {}
    for name, s in configs.items():
        pcm = d_pcm if s.audio_channels else None
        p = strmux.plan(s, n, per_ch if s.audio_channels else 0)
        state[name] = dict(s=s, pcm=pcm, plan=p, mux=strmux.StrMuxer((0,)),
                           out=torch.zeros((S, p.n_sectors, p.sector_size), dtype=torch.uint8, device=dev), ms=[])
    torch.cuda.synchronize()
    for st in state.values():
        for _ in range(args.warmup):
            st["mux"].encode_device(st["s"], d_frames, st["pcm"], d_out=st["out"])
    for _ in range(args.rounds):
        for st in state.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st["mux"].encode_device(st["s"], d_frames, st["pcm"], d_out=st["out"])
            torch.cuda.synchronize()
            st["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
    result = {"tool": "tools/gpu_strspu_bench.py", "streams_per_call": S, "frames_per_stream": n, "steps_per_round": args.steps, "rounds": args.rounds,
              "gpu": torch.cuda.get_device_name(0), "version": L.psxhip_version().decode(), "adpcm_kernel_rev": L.psxhip_adpcm_kernel_rev().decode(),
              "strspu_kernel_rev": strmux.strspu_kernel_rev(), "adpcm_chunked_threshold": int(L.psxhip_adpcm_chunked_threshold(2 * S)), "configs": {}}
    for name, st in state.items():
        p, med = st["plan"], statistics.median(st["ms"])
        units = (p.n_audio_sectors * (63 if name == "strspu" else 72) - (1 if name == "strspu" else 0)) if p.n_audio_sectors else 0
        result["configs"][name] = {
            "n_sectors": p.n_sectors, "n_audio_sectors": p.n_audio_sectors, "sector_size": p.sector_size, "units_per_chain": units,
            "ms_per_call_rounds": [round(v, 4) for v in st["ms"]], "ms_per_call_median": round(med, 4),
            "sectors_per_sec": round(p.n_sectors * S / (med * 1e-3), 1), "frames_per_sec": round(n * S / (med * 1e-3), 1),
            "sha256_stream0": hashlib.sha256(st["out"][0].cpu().numpy().tobytes()).hexdigest()}
        st["mux"].close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
