#!/usr/bin/env python3
"""Times the disc finisher (psxhip_disc_finish_device) and its check (psxhip_disc_check_device) on config 5's sector count -- 8 XA
channels x 60 minutes = 540 000 sectors, 8 sources of 2336-byte sectors at period 8 -- resident in HBM, once with form-2 (XA sound)
sources and once with the same bytes as form-1 sources, beside a device-to-device copy of the image's bytes in the same run.

  python tools/gpu_disc_bench.py --out profiles/<kernel rev>_bench.json

540 000 sectors are more than one disc addresses (lba + 150 stays below 450 000), so the job is two discs of 270 000 sectors: two calls,
timed as one.  HIP events around each leg, every leg warmed up first, the legs alternated inside each repeat, the minimum over the
repeats.  Prints one JSON line: sectors/s, GB/s of algorithmic bytes (2336 read + 2352 written per sector; the check: 2352 read), that
as a fraction of 8 TB/s, and the time as a ratio to the copy's.  Needs the GPU: there is no fallback.  Counters come from a run of
their own: `rocprofv3 --pmc ... -- python tools/gpu_disc_bench.py --repeats 1 --sectors 67500`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sectors", type=int, default=540000, help="sectors of the whole job (a multiple of 16)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "gpu_disc_bench needs an MI355X"
    from psxavenc_amd import disc

    dev = torch.device("cuda:0")
    n, discs, period = args.sectors, 2, 8
    assert n % (discs * period) == 0
    per_disc = n // discs
    per_source = per_disc // period
    g = torch.Generator(device=dev).manual_seed(5)
    d_src = torch.randint(0, 256, (discs, period, per_source, 2336), generator=g, dtype=torch.int32, device=dev).to(torch.uint8)
    d_img = torch.empty((discs, per_disc, 2352), dtype=torch.uint8, device=dev)
    d_copy = torch.empty_like(d_img)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def set_form(submode):
        d_src[..., 2] = submode
        d_src[..., 4:8] = d_src[..., 0:4]

    lay = disc.layout(list(range(period)), 0)
    tables = [[disc.source(d_src[k, s], channel=s) for s in range(period)] for k in range(discs)]

    def finish():
        for k in range(discs):
            disc.disc_finish(lay, tables[k], 0, per_disc, d_out=d_img[k])

    def check():
        return [disc.disc_check(d_img[k], 0, status=False)[1] for k in range(discs)]

    record = {"kernel_rev": disc.kernel_rev(), "device": torch.cuda.get_device_name(0), "sectors": n, "repeats": args.repeats,
              "job": "%d discs of %d sectors, 8 sources of 2336-byte sectors at period 8" % (discs, per_disc),
              "method": "HIP events around each leg, legs alternated, minimum over the repeats; GB/s of algorithmic bytes: finish 2336 read + "
                        "2352 written per sector, check 2352 read, copy 2352 read + 2352 written"}
    for name, submode in (("form2", 0x64), ("form1", 0x48)):
        set_form(submode)
        finish(), check(), d_copy.copy_(d_img)          # warm-up
        torch.cuda.synchronize()
        t = {"finish": [], "check": [], "copy": []}
        for _ in range(args.repeats):
            t["finish"].append(timed(finish)[0])
            ms, sums = timed(check)
            t["check"].append(ms)
            t["copy"].append(timed(lambda: d_copy.copy_(d_img))[0])
        total = sum(s.cpu() for s in sums).tolist()
        want_forms = [n, 0] if name == "form1" else [0, n]
        assert total[0] == n and total[1:3] == want_forms and total[3] == 0, "the finished image does not check clean: %s" % total
        copy_s = min(t["copy"]) / 1e3
        leg = {}
        for what, per_sector in (("finish", 2336 + 2352), ("check", 2352), ("copy", 2 * 2352)):
            s = min(t[what]) / 1e3
            leg[what] = {"ms": round(s * 1e3, 4), "sectors_per_s": round(n / s), "GB_per_s": round(n * per_sector / s / 1e9, 1),
                         "fraction_of_8TBps": round(n * per_sector / s / PEAK_BYTES_PER_S, 4), "time_over_copy": round(s / copy_s, 3),
                         "ms_all": [round(x, 4) for x in t[what]]}
        record[name] = leg
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
