#!/usr/bin/env python3
"""Times a sound bank of 1000 entries of 0.1 .. 2 s at 22050 Hz (tones and noise) through three encoders:

  one psxhip_spu_bank_encode_device call          (device events and wall clock; PCM and bank stay in HBM)
  a loop of psxhip_spu_file_encode_host calls     (wall clock; PCM from host memory, one file per call)
  the reference build's psx_audio_spu_encode      (wall clock, one core; oracle/_ref, or the project's oracle where that is absent)

and the same bank with its entries listed longest-first against entry order (the chains kernel runs four chains per wavefront to the
longest of the four: sorting groups chains of like length; the files cannot differ).

  python tools/gpu_spu_bank_probe.py --out profiles/<kernel rev>_probe.json

Every shape is warmed up first; median [min, max] over the repeats.  Needs the GPU: there is no fallback."""
import argparse
import ctypes as C
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
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "gpu_spu_bank_probe needs an MI355X"
    import oracle_lib as O
    from psxavenc_amd import SpuBank, spubank, spufile

    rng = np.random.default_rng(2024)
    freq, n = 22050, args.entries
    lengths = rng.integers(freq // 10, 2 * freq + 1, n)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    total_samples = int(lengths.sum())
    t = np.arange(total_samples)
    pcm = (9000 * np.sin(2 * np.pi * 440 * t / freq) + 5000 * np.sin(2 * np.pi * 1733 * t / freq) + rng.normal(0, 1500, total_samples)).astype(np.int16)
    s = spubank.settings(spufile.FORMAT_VAG, 64, False, 16)

    def entries_in(order):
        return [spubank.entry(int(offsets[i]), int(lengths[i]), freq, 50 if i % 2 else -1, i % 3 == 0, "s%04d" % i) for i in order]

    def med(v):
        return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]

    d_pcm = torch.from_numpy(pcm).to("cuda:0")
    legs = {}
    banks = {}
    for label, order in (("entry order", list(range(n))), ("longest first", [int(i) for i in np.argsort(-lengths, kind="stable")])):
        bank = SpuBank(s, entries_in(order), device=0)
        d_out = bank.encode_device(d_pcm)
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            bank.encode_device(d_pcm, d_out)
            b.record()
            b.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
        assert not bank.check_device(d_out).any()
        file_offsets, sizes, total = bank.layout()
        host = d_out.cpu().numpy()
        banks[label] = {order[k]: host[file_offsets[k]:file_offsets[k] + sizes[k]].copy() for k in range(n)}
        legs["encode_device, " + label] = {"device_ms": med(ev), "wall_ms": med(wall), "bank_bytes": total}
        bank.close()
    assert all(np.array_equal(banks["entry order"][i], banks["longest first"][i]) for i in range(n)), "the order of the chain table changed a file"

    wall = []
    for r in range(args.host_repeats + 1):
        t0 = time.perf_counter()
        for i in range(n):
            one = spufile.settings(spufile.FORMAT_VAG, 1, freq, alignment=64, loop_point=50 if i % 2 else -1, enable_loop=i % 3 == 0, name="s%04d" % i)
            f = spufile.encode(one, pcm[offsets[i]:offsets[i] + lengths[i]])
            if r == 0:
                assert np.array_equal(f, banks["entry order"][i]), "psxhip_spu_file_encode_host and the bank differ at entry %d" % i
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
    legs["loop of psxhip_spu_file_encode_host"] = {"wall_ms": med(wall)}

    R = O.ref()
    t0 = time.perf_counter()
    for i in range(n):
        x = np.ascontiguousarray(pcm[offsets[i]:offsets[i] + lengths[i]])
        out = np.zeros(-(-len(x) // 28) * 16, np.uint8)
        if R is not None:
            R.psx_audio_spu_encode(C.byref(O.RefChan()), O.ptr(x, O.i16p), len(x), 1, O.ptr(out, O.u8p))
        else:
            O.lib().orc_spu_encode(C.byref(O.Chan(0, 0)), O.ptr(x, O.i16p), len(x), 1, O.ptr(out, O.u8p))
    legs["reference encoder, one core"] = {"wall_ms": [round((time.perf_counter() - t0) * 1e3, 3)] * 3,
                                           "encoder": "oracle/_ref (libpsxav, unchanged)" if R is not None else "oracle/adpcm_oracle.c (no reference build here)"}

    blocks = int(sum(-(-int(v) // 28) for v in lengths))
    record = {"kernel_rev": spubank.kernel_rev(), "device": torch.cuda.get_device_name(0),
              "job": "%d entries of 0.1 .. 2 s at %d Hz, VAG, alignment 64: %d samples, %d blocks" % (n, freq, total_samples, blocks),
              "method": "median [min, max] milliseconds over %d repeats (host loop: %d), every shape warmed up; device_ms from events around the call"
              % (args.repeats, args.host_repeats), "legs": legs,
              "microseconds_per_block": {k: round(1e3 * v.get("device_ms", v["wall_ms"])[0] / blocks, 4) for k, v in legs.items()}}
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
