#!/usr/bin/env python3
"""Round-5 diagnostics of the frame kernel off the friendly point (GPU box).
For each content class (a4 = the headline's noise +-4, a8 = noise +-8: answers flip between scales 5 and 6, mixed = the
scene-structured sequence of psxavenc_amd/mixed.py): frames/s for one 1000-frame launch at a time (one lane, two lanes), for the
four batches as one batch list, for a cold context; and -- from the diagnostics instantiation -- passes per frame, how often the
first guess was right, where a group's time goes and how far apart the groups end.
usage: python tools/gpu_r05_diag.py [a4 a8 mixed ...] [--json out.json]"""
import collections
import ctypes as C
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from psxavenc_amd import _lib, mixed, synth
from psxavenc_amd.mdec import MdecEncoder

W, H, BUDGET, N, CODEC = 320, 240, 8192, 1000, 0
NT = 8 + 4 * 1024 + 16 + 2048
SHAPES = {"v3a4": (1, 640, 480, 8192, 1250, 4), "v3a8_32k": (1, 640, 480, 32768, 1250, 8), "v2_16k": (0, 320, 240, 16128, 1000, 4)}


def batches(kind):
    global W, H, BUDGET, N, CODEC
    if kind == "mixed":
        CODEC, W, H, BUDGET, N = 0, 320, 240, 8192, 1000
        whole = mixed.frames_device(W, H, 1, 0, 4 * N, device=0)
        return [whole[i * N:(i + 1) * N] for i in range(4)]
    if kind in SHAPES:
        CODEC, W, H, BUDGET, N, amp = SHAPES[kind]
    else:
        CODEC, W, H, BUDGET, N = 0, 320, 240, 8192, 1000
        amp = int(kind[1:])
    return [synth.frames_device(W, H, 101 + b, 0, N, amp, device=0) for b in range(4)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for k in range(reps):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def rates(bb):
    outs = [(torch.zeros((N, BUDGET), dtype=torch.uint8, device="cuda"), torch.zeros((N, 4), dtype=torch.int32, device="cuda")) for _ in range(4)]
    r = {}
    for lanes in (1, 2):
        enc = MdecEncoder(CODEC, W, H, max_frame_size=BUDGET, device=0)
        if lanes > 1:
            enc.set_lanes(lanes)

        def one(k):
            enc.encode_frames_device(bb[k % 4], BUDGET, d_out=outs[k % 4][0], d_results=outs[k % 4][1])
        timed(one, 8)
        enc.fence()
        ms = min(timed(lambda k: (one(k), enc.fence() if k == 63 else None), 64) for _ in range(3))
        r["lanes%d" % lanes] = {"frames_per_sec": round(N / ms * 1e3), "ms_per_launch": round(ms, 5)}
        enc.close()
    enc = MdecEncoder(CODEC, W, H, max_frame_size=BUDGET, device=0)
    lst = [(bb[i], outs[i][0], outs[i][1]) for i in range(4)]
    timed(lambda k: enc.encode_batches_device(lst, BUDGET), 3)
    ms = min(timed(lambda k: enc.encode_batches_device(lst, BUDGET), 16) for _ in range(3))
    r["batch_list_4x1000"] = {"frames_per_sec": round(4 * N / ms * 1e3), "ms_per_launch": round(ms, 5)}
    enc.close()
    cold = []
    for t in range(5):
        enc = MdecEncoder(CODEC, W, H, max_frame_size=BUDGET, device=0)
        cold.append(timed(lambda k: enc.encode_frames_device(bb[t % 4], BUDGET, d_out=outs[0][0], d_results=outs[0][1]), 1))
        enc.close()
    cold.sort()
    r["cold_first_launch"] = {"frames_per_sec": round(N / cold[2] * 1e3), "ms_median": round(cold[2], 5), "ms_min": round(cold[0], 5)}
    # cold, the way the headline is measured: a fresh context, two lanes, its first four launches (four different batches) back to back
    cold2 = []
    for t in range(5):
        enc = MdecEncoder(CODEC, W, H, max_frame_size=BUDGET, device=0)
        enc.set_lanes(2)
        cold2.append(timed(lambda k: (enc.encode_frames_device(bb[k % 4], BUDGET, d_out=outs[k % 4][0], d_results=outs[k % 4][1]), enc.fence() if k == 3 else None), 4))
        enc.close()
    cold2.sort()
    r["cold_first_4_launches_two_lanes"] = {"frames_per_sec": round(N / cold2[2] * 1e3), "ms_per_launch_median": round(cold2[2], 5)}
    sc = collections.Counter()
    for o in outs:
        s, c = o[1][:, 0].cpu().unique(return_counts=True)
        for a, b in zip(s.tolist(), c.tolist()):
            sc[int(a)] += int(b)
    r["quant_scale_hist_4000_frames"] = {str(k): v for k, v in sorted(sc.items())}
    return r


def stats_run(bb, warm):
    os.environ["PSXHIP_MDEC_STATS"] = "1"
    enc = MdecEncoder(CODEC, W, H, max_frame_size=BUDGET, device=0)
    del os.environ["PSXHIP_MDEC_STATS"]
    out = torch.zeros((N, BUDGET), dtype=torch.uint8, device="cuda")
    res = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    L = _lib.lib()
    t = (C.c_ulonglong * NT)()
    for k in range(warm):
        enc.encode_frames_device(bb[k % 4], BUDGET, d_out=out, d_results=res)
    torch.cuda.synchronize()
    L.psxhip_mdec_read_stats(enc._h, t, NT, 1)
    enc.encode_frames_device(bb[warm % 4], BUDGET, d_out=out, d_results=res)
    torch.cuda.synchronize()
    L.psxhip_mdec_read_stats(enc._h, t, NT, 1)
    s = list(t)
    enc.close()
    r = {"frames": s[0], "passes_per_frame": round(s[1] / max(1, s[0]), 4), "passes_hist_0_1_2_3_4_5plus": s[2:8]}
    fr = np.array(s[8 + 4096 + 16:8 + 4096 + 16 + N], dtype=np.int64)
    guess, ab, ans, np_ = fr & 0xFF, (fr >> 8) & 0x7F, (fr >> 16) & 0xFF, (fr >> 24) & 0xFF
    r["last_pass_stopped_counting_at_its_checkpoint"] = int(((fr >> 15) & 1).sum())      # (v2, mdec-k3.9: the count became a mixed bound)
    tr = ["/".join(("%d%s%s" % (b & 0x3F, "c" if b & 0x40 else "", "!" if b & 0x80 else "")) for b in [(int(x) >> (32 + 8 * k)) & 0xFF for k in range(4)] if b) for x in fr]
    r["first_guess_right"] = int((guess == ans).sum())
    r["first_guess_off_by_one"] = int((np.abs(guess - ans) == 1).sum())
    r["first_guess_off_by_more"] = int((np.abs(guess - ans) > 1).sum())
    r["stopped_at_checkpoint"] = int((ab != 0).sum())
    dd = np.clip(guess - ans, -4, 4)
    r["first_guess_minus_answer_hist_-4..+4"] = np.bincount(dd + 4, minlength=9).tolist()
    hi = ans >= 8
    r["first_guess_minus_answer_hist_answers_8_and_up"] = np.bincount(dd[hi] + 4, minlength=9).tolist()
    c = collections.Counter(zip(guess.tolist(), ab.tolist(), ans.tolist(), np_.tolist()))
    r["top_cases_guess_abort_answer_passes_count"] = [list(k) + [v] for k, v in sorted(c.items(), key=lambda x: -x[1])[:10]]
    r["cases_with_3_or_more_passes"] = [list(k) + [v] for k, v in sorted(c.items(), key=lambda x: -x[0][3] * 1000 - x[1]) if k[3] >= 3][:16]
    c2 = collections.Counter(zip(guess.tolist(), ab.tolist(), ans.tolist(), np_.tolist(), tr))
    r["pass_traces_of_frames_with_3_or_more_passes"] = [list(k) + [v] for k, v in sorted(c2.items(), key=lambda x: -x[0][3] * 1000 - x[1]) if k[3] >= 3][:24]
    ph = np.array(s[8 + 4096:8 + 4096 + 16], dtype=np.float64)
    r["phase_share_pct_ticket_resetdc_pilot_passes_scanmerge_writeout"] = np.round(100 * ph[:6] / max(1.0, ph[:6].sum()), 1).tolist()
    r["barrier_wait_pct_of_residency"] = round(100.0 * ph[6] / max(1.0, ph[7]), 1)
    a = np.array(s[8:8 + 4096], dtype=np.int64).reshape(-1, 4)
    a = a[a[:, 1] > 0]
    if len(a):
        t0 = a[:, 0].min()
        st, en, nf = (a[:, 0] - t0) / 100.0, (a[:, 1] - t0) / 100.0, a[:, 2] & 0xFF
        r["groups"] = int(len(a))
        r["group_end_us_min_p10_p50_p90_max"] = [round(float(x), 1) for x in (en.min(), np.percentile(en, 10), np.percentile(en, 50), np.percentile(en, 90), en.max())]
        r["mean_residency_pct_of_span"] = round(float(100 * (en - st).mean() / en.max()), 1)
        r["frames_per_group_hist"] = np.bincount(nf).tolist()
    return r


def main():
    argv = sys.argv[1:]
    json_out = None
    if "--json" in argv:
        i = argv.index("--json")
        json_out = argv[i + 1]
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    kinds = args or ["a4", "a8", "mixed"]
    res = {"library": _lib.lib().psxhip_version().decode()}
    for kind in kinds:
        bb = batches(kind)
        torch.cuda.synchronize()
        res[kind] = {"rates": rates(bb), "warm_launch": stats_run(bb, 5), "cold_launch": stats_run(bb, 0)}
        print(kind, json.dumps(res[kind]), flush=True)
    if json_out:
        with open(json_out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
