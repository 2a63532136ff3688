#!/usr/bin/env python3
"""Times the disc reader (psxhip_disc_read_device) on a clean finished image of one disc -- 270 000 sectors, 8 sources of 2336-byte
sectors at period 8, read into 8 tracks of 2336-byte sectors -- resident in HBM, once as form 1 and once as form 2, beside the
check (psxhip_disc_check_device) on the same image and a device-to-device copy of the image's bytes, in the same run.

  python tools/gpu_disc_read_bench.py --out profiles/<kernel rev>_bench.json

HIP events around each leg, every leg warmed up first, the legs alternated inside each repeat, the minimum over the repeats.  Prints
one JSON line: sectors/s, GB/s of algorithmic bytes (read: 2352 read twice and 2336 written per sector; check: 2352 read; copy: 2352
read and 2352 written), and the read's time as a ratio to the check's, to the copy's and to their sum.  A clean image is the fast
path: no sector enters a second round.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sectors", type=int, default=270000, help="sectors of the image (a multiple of 8)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "gpu_disc_read_bench needs an MI355X"
    from psxavenc_amd import disc, discread

    dev = torch.device("cuda:0")
    n, period = args.sectors, 8
    assert n % period == 0
    per_source = n // period
    g = torch.Generator(device=dev).manual_seed(5)
    d_src = torch.randint(0, 256, (period, per_source, 2336), generator=g, dtype=torch.int32, device=dev).to(torch.uint8)
    d_img = torch.empty((n, 2352), dtype=torch.uint8, device=dev)
    d_copy = torch.empty_like(d_img)
    d_tracks = torch.zeros((period, per_source, 2336), dtype=torch.uint8, device=dev)
    reader = discread.DiscReader(0)
    tracks = [discread.track(d_tracks[s], file=1, channel=s) for s in range(period)]
    lay = disc.layout(list(range(period)), 0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def read():
        return reader.read_device(d_img, tracks, table=False)

    def check():
        return disc.disc_check(d_img, 0, status=False)[1]

    record = {"kernel_rev": discread.kernel_rev(), "check_kernel_rev": disc.kernel_rev(), "device": torch.cuda.get_device_name(0),
              "sectors": n, "repeats": args.repeats, "job": "a clean image of %d sectors, 8 tracks of 2336-byte sectors at period 8" % n,
              "method": "HIP events around each leg, legs alternated, minimum over the repeats; GB/s of algorithmic bytes: read 2 x 2352 "
                        "read + 2336 written per sector, check 2352 read, copy 2352 read + 2352 written"}
    for name, submode in (("form1", 0x48), ("form2", 0x64)):
        d_src[..., 0], d_src[..., 2] = 1, submode
        d_src[..., 4:8] = d_src[..., 0:4]
        disc.disc_finish(lay, [disc.source(d_src[s], channel=s) for s in range(period)], 0, n, d_out=d_img)
        d_tracks.zero_()
        read(), check(), d_copy.copy_(d_img)            # warm-up
        torch.cuda.synchronize()
        t = {"read": [], "check": [], "copy": []}
        for _ in range(args.repeats):
            ms, out = timed(read)
            t["read"].append(ms)
            t["check"].append(timed(check)[0])
            t["copy"].append(timed(lambda: d_copy.copy_(d_img))[0])
        s = discread.summary_dict(out["summary"].cpu().tolist())
        want = dict.fromkeys(discread.SUMMARY_FIELDS, 0)
        want.update(n_sectors=n, n_form1=n if name == "form1" else 0, n_form2=n if name == "form2" else 0, n_clean=n if name == "form1" else 0)
        assert s == want and out["counts"].cpu().tolist() == [per_source] * period, "the clean image does not read clean: %s" % s
        body = d_img.view(per_source, period, 2352)[:, :, 0x10:].transpose(0, 1)
        assert torch.equal(d_tracks, body), "a track is not the image's sectors of its channel"
        check_s, copy_s = min(t["check"]) / 1e3, min(t["copy"]) / 1e3
        leg = {}
        for what, per_sector in (("read", 2 * 2352 + 2336), ("check", 2352), ("copy", 2 * 2352)):
            sec = min(t[what]) / 1e3
            leg[what] = {"ms": round(sec * 1e3, 4), "sectors_per_s": round(n / sec), "GB_per_s": round(n * per_sector / sec / 1e9, 1),
                         "ms_all": [round(x, 4) for x in t[what]]}
        read_s = min(t["read"]) / 1e3
        leg["read_over_check"] = round(read_s / check_s, 3)
        leg["read_over_copy"] = round(read_s / copy_s, 3)
        leg["read_over_check_plus_copy"] = round(read_s / (check_s + copy_s), 3)
        record[name] = leg
    reader.close()
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
