#!/usr/bin/env python3
"""Times "psxhip SPU loop seam v1"  on the 1000-entry bank of tools/gpu_spu_bank_probe.py (0.1 .. 2 s at
22050 Hz, VAG, alignment 64), every entry made a loop: enable_loop, a loop point somewhere in its first half, and material that is
exactly periodic over the body (three partials with whole numbers of cycles, and noise that repeats with the body).

  psxhip_spu_bank_encode_device with the seam mode off and on   (device events around the call, warmed, median of 7)
  the outcome per entry                                         (histogram of the pass numbers)
  psxhip_spu_bank_seam_device on both banks                     (its time with and without PCM; the sums of pass1_err and pass2_err and
                                                                 their change in dB)

  python tools/gpu_spu_seam_probe.py --out profiles/<kernel rev>_probe.json

Needs the GPU: there is no fallback."""
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
    ap.add_argument("--entries", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "gpu_spu_seam_probe needs an MI355X"
    from psxavenc_amd import SpuBank, spubank, spufile

    rng = np.random.default_rng(2024)
    freq, n = 22050, args.entries
    lengths = rng.integers(freq // 10, 2 * freq + 1, n)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    loop_ms = [int(rng.integers(0, 500 * int(v) // freq)) for v in lengths]
    pcm = np.zeros(int(lengths.sum()), np.int16)
    for i in range(n):
        first = 28 * (loop_ms[i] * freq // 28000)
        body = int(lengths[i]) - first
        k = np.arange(int(lengths[i])) - first
        x = np.zeros(int(lengths[i]))
        for cycles, amp in zip(rng.integers(1, max(2, body // 40), 3), (9000, 5000, 2000)):
            x += amp * np.sin(2 * np.pi * int(cycles) * k / body + rng.uniform(0, 2 * np.pi))
        x += rng.normal(0, 1500 if i % 2 else 100, body)[k % body]
        pcm[offsets[i]:offsets[i] + lengths[i]] = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    s = spubank.settings(spufile.FORMAT_VAG, 64, False, 16)
    entries = [spubank.entry(int(offsets[i]), int(lengths[i]), freq, loop_ms[i], True, "s%04d" % i) for i in range(n)]

    def med(v):
        return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]

    def timed(call):
        call()
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b))
        return med(ev)

    d_pcm = torch.from_numpy(pcm).to("cuda:0")
    bank = SpuBank(s, entries, device=0)
    legs, banks, reports = {}, {}, {}
    for label, mode in (("seam mode off", spubank.SEAM_OFF), ("seam mode steady", spubank.SEAM_STEADY)):
        bank.set_seam(mode)
        d_out = bank.encode_device(d_pcm)
        legs["encode_device, " + label] = {"device_ms": timed(lambda: bank.encode_device(d_pcm, d_out))}
        assert not bank.check_device(d_out).any()
        banks[label] = d_out
        legs["seam_device, bank of " + label] = {"device_ms": timed(lambda: bank.seam_report(d_out, d_pcm))}
        legs["seam_device without PCM, bank of " + label] = {"device_ms": timed(lambda: bank.seam_report(d_out))}
        reports[label] = bank.seam_records(bank.seam_report(d_out, d_pcm))
    outcome = bank.seam_passes().cpu().numpy()
    bank.close()

    off, on = reports["seam mode off"], reports["seam mode steady"]
    assert (off["seam_block"] >= 0).all() and np.array_equal(off["seam_block"], on["seam_block"])
    fixed = (outcome > 0) & (outcome < spubank.SEAM_PASSES)

    def db(a, b):
        return round(float(10 * np.log10(float(a) / float(b))), 3) if a and b else None
    gains = [10 * np.log10(float(a) / float(b)) for a, b in zip(off["pass2_err"][fixed], on["pass2_err"][fixed]) if a and b]
    blocks = int(sum(-(-int(v) // 28) for v in lengths))
    record = {
        "kernel_rev": spubank.seam_kernel_rev(), "bank_kernel_rev": spubank.kernel_rev(), "device": torch.cuda.get_device_name(0),
        "job": "%d looping entries of 0.1 .. 2 s at %d Hz, VAG, alignment 64, material periodic over the body: %d samples, %d blocks"
               % (n, freq, int(lengths.sum()), blocks),
        "method": "median [min, max] milliseconds over %d repeats from events around the call, every call warmed up" % args.repeats,
        "passes": spubank.SEAM_PASSES, "legs": legs,
        "steady_over_off": round(legs["encode_device, seam mode steady"]["device_ms"][0] / legs["encode_device, seam mode off"]["device_ms"][0], 3),
        "pass_histogram": {str(k): int((outcome == k).sum()) for k in range(-1, spubank.SEAM_PASSES + 1)},
        "entries_changed": int(fixed.sum()),
        "settled": {"off": int(off["settled"].sum()), "steady": int(on["settled"].sum()), "steady, fixed behind pass 0": int(on["settled"][fixed].sum())},
        "sum_pass1_err": {"off": int(off["pass1_err"].sum()), "steady": int(on["pass1_err"].sum())},
        "sum_pass2_err": {"off": int(off["pass2_err"].sum()), "steady": int(on["pass2_err"].sum())},
        "pass1_err_change_db": db(on["pass1_err"].sum(), off["pass1_err"].sum()),
        "pass2_err_change_db": db(on["pass2_err"].sum(), off["pass2_err"].sum()),
        "pass2_gain_db_of_changed_entries": {"median": round(float(np.median(gains)), 3), "min": round(float(min(gains)), 3),
                                             "max": round(float(max(gains)), 3)} if gains else None,
    }
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
