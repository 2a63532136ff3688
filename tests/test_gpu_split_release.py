"""The split kernel's release path (csrc/mdec_split.inc): a frame whose workgroups do not all arrive is given up by the watchdog.

Two test switches make that happen on demand, read when a context is created: PSXHIP_MDEC_SPLIT_WITHHOLD=frame:segment[:launches
[:residue]] (every other group reads that segment's words as never there, without waiting; with `residue` the withheld group leaves
what a late group leaves) and PSXHIP_MDEC_SPLIT_PATIENCE=<ticks> (real releases and real late groups on an idle GPU).  Against the
CPU oracle, byte for byte:
  * the host-buffer paths (one-frame calls, encode_frames_host, the STR calls, the multi-device call) return the exact frame;
  * the device path reports PSXHIP_MDEC_QS_RELEASED with a zero row for the withheld frame only, 64 still means "fits nowhere";
  * nothing a launch leaves in the workspace changes a later launch's bytes or results (sizes 1 -> 12 -> 3 -> 1, one lane, two
    lanes, the one-frame workspace);
  * psxhip_mdec_watchdog counts each released frame once;
  * short patience and co-tenant processes: host results exact, device results exact or released.
Children run this file as a script (the switches are per context, and co-tenants are processes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import oracle_lib as O  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, BUDGET = 320, 240, 8192
RELEASED = 65
SEGS = ["0", "mid", "-1"]          # the first segment, a middle one, the finisher's own


def _ctx(codec, budget=BUDGET, w=W, h=H, **env):
    """an MdecEncoder created with the given switches in the environment (they are read when the context is created)"""
    from psxavenc_amd.mdec import MdecEncoder
    with _env(**env):
        return MdecEncoder(codec, w, h, max_frame_size=budget, device=0)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(out, res, want, want_res, tag):
    assert np.array_equal(res, want_res), (tag, res.tolist(), want_res.tolist())
    bad = np.nonzero((out[:, :want.shape[1]] != want).any(axis=1))[0]
    assert bad.size == 0, "%s: frames %s differ" % (tag, bad.tolist())


def _frames(n, seed, amp=6):
    return O.synth_frames(W, H, n, seed=seed, amp=amp)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_withheld_segment_host_paths_return_the_exact_frame(codec, seg):
    """one-frame calls and 2 / 5 / 12-frame encode_frames_host with frame 0 withheld in every split launch: every frame equals the
    oracle (not ENOFIT), and the watchdog goes up by one per launch"""
    enc = _ctx(codec, PSXHIP_MDEC_SPLIT_WITHHOLD="0:%s:1000" % seg)
    launches = 0
    for n, seed in ((1, 3), (1, 4), (2, 5), (5, 6), (12, 7), (1, 8)):
        fr = _frames(n, seed)
        want, want_res, rc = O.mdec_encode(codec, W, H, fr, BUDGET)
        assert rc == 0
        out, res = enc.encode_frames_host(fr, BUDGET)
        _same(out, res, want, want_res, "codec %d seg %s n=%d" % (codec, seg, n))
        launches += 1
        assert enc.watchdog() == launches, (n, enc.watchdog(), launches)
    # encode_frame_bs, the reference's call
    fr = _frames(1, 9)
    want, want_res, _ = O.mdec_encode(codec, W, H, fr, BUDGET)
    enc.frame_max_size = BUDGET
    enc.encode_frame_bs(fr[0])
    assert enc.quant_scale == want_res[0, 0] and np.array_equal(enc.frame_output, want[0])
    assert enc.watchdog() == launches + 1
    enc.close()


@pytest.mark.parametrize("codec", [0, 1, 2])
def test_withheld_segment_str_and_multi_device_paths(codec):
    """psxhip_str_encode_device / _host on a 10-frame stream against the reference loop, and a multi-device list of one entry,
    with frame 0 withheld in every split launch of the contexts they create"""
    import torch
    import str_reference_loop as R
    from psxavenc_amd import strmux
    from psxavenc_amd.multi import MdecMulti
    fmt, n_frames, channels = 7, 10, 2
    s = strmux.settings(fmt=fmt, codec=codec, width=W, height=H, channels=channels, frequency=37800, bits=4)
    frames = _frames(n_frames, 31)
    pl = strmux.plan(s, n_frames)
    n = (pl.n_audio_sectors + 2) * pl.audio_samples_per_sector + 100
    pcm = np.zeros(n * channels, np.int16)
    for c in range(channels):
        pcm[c::channels] = O.synth_pcm(9, c, 0, n, 0)
    want, qsum, frames_encoded = R.encode_file_str(fmt, codec, W, H, 15, 1, 2, frames, pcm, channels=channels)
    for seg in SEGS:
        with _env(PSXHIP_MDEC_SPLIT_WITHHOLD="0:%s:1000" % seg):
            mux = strmux.StrMuxer((0,))
            d_out, p = mux.encode_device(s, torch.from_numpy(frames).to("cuda:0"), torch.from_numpy(pcm).to("cuda:0"))
            host, ph = mux.encode(s, frames, pcm)
        got = d_out.cpu().numpy()[0]
        assert got.shape == want.shape
        for name, g, pp in (("device", got, p), ("host", host, ph)):
            bad = np.nonzero((g != want).any(axis=1))[0]
            assert bad.size == 0, "codec %d seg %s %s: sectors differ: %s" % (codec, seg, name, bad[:8].tolist())
            assert pp.quant_scale_sum == qsum and pp.n_frames_encoded == frames_encoded, (name, seg)
        mux.close()
        fr = _frames(5, 32)
        want_f, want_res, rc = O.mdec_encode(codec, W, H, fr, BUDGET)
        assert rc == 0
        with _env(PSXHIP_MDEC_SPLIT_WITHHOLD="0:%s:1000" % seg):
            m = MdecMulti((0,), codec, W, H, max_frame_size=BUDGET)
        out, res = m.encode_frames_host(fr, BUDGET)
        _same(out, res, want_f, want_res, "multi codec %d seg %s" % (codec, seg))
        m.close()


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_withheld_segment_device_path_reports_released(codec, seg):
    """encode_frames_device: the withheld frame comes back as PSXHIP_MDEC_QS_RELEASED with a zero row, every other frame is exact,
    and a frame whose budget is below the floor (no scale can fit: two end-of-block bits per block alone are 450 bytes) still says 64"""
    import torch
    n = 5
    fr = _frames(n, 41)
    budgets = np.array([BUDGET, 6000, 400, BUDGET, 7001], np.int32)
    assert O.mdec_encode(codec, W, H, fr[2:3], 400)[2] != 0
    enc = _ctx(codec, PSXHIP_MDEC_SPLIT_WITHHOLD="1:%s:1" % seg)
    d_out, d_res = enc.encode_frames_device(torch.from_numpy(fr).to("cuda:0"), torch.from_numpy(budgets).to("cuda:0"))
    torch.cuda.synchronize()
    out, res = d_out.cpu().numpy(), d_res.cpu().numpy()
    assert enc.watchdog() == 1
    assert res[1].tolist() == [RELEASED, 0, 0, 0] and not out[1].any(), (codec, seg, res[1].tolist())
    assert res[2].tolist() == [64, 0, 0, 0] and not out[2].any(), (codec, seg, res[2].tolist())
    for k in (0, 3, 4):
        want, want_res, rc = O.mdec_encode(codec, W, H, fr[k:k + 1], int(budgets[k]))
        assert rc == 0
        _same(out[k:k + 1, :budgets[k]], res[k:k + 1], want, want_res, "codec %d seg %s frame %d" % (codec, seg, k))
    # the next launch (no switch any more) is exact for every frame
    d_out, d_res = enc.encode_frames_device(torch.from_numpy(fr[[0, 1, 3]]).to("cuda:0"), BUDGET)
    torch.cuda.synchronize()
    want, want_res, rc = O.mdec_encode(codec, W, H, fr[[0, 1, 3]], BUDGET)
    _same(d_out.cpu().numpy(), d_res.cpu().numpy(), want, want_res, "codec %d seg %s after" % (codec, seg))
    assert enc.watchdog() == 1
    enc.close()


@pytest.mark.parametrize("first", [1, 12])
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("codec", [0, 1, 2])
def test_residue_of_a_released_launch_changes_no_later_launch(codec, seg, first):
    """one launch whose withheld group leaves its round-0 sums, DC words and done = 2 behind (what a late group leaves), then normal
    launches of 1, 12, 3, 1 frames on the same workspace -- one lane, two lanes -- and one-frame calls on the one-frame workspace:
    all exact, and the watchdog counts the one release only"""
    import torch
    fr = _frames(first + 17, 51, amp=7)
    want, want_res, rc = O.mdec_encode(codec, W, H, fr, BUDGET)
    assert rc == 0
    d = torch.from_numpy(fr).to("cuda:0")
    for lanes in (1, 2):
        enc = _ctx(codec, PSXHIP_MDEC_SPLIT_WITHHOLD="0:%s:1:1" % seg)
        if lanes > 1:
            enc.set_lanes(2)
        runs, at = [], 0
        for n in (first, 1, 12, 3, 1):
            o, r = enc.encode_frames_device(d[at:at + n], BUDGET)
            runs.append((at, n, o, r))
            at += n
        enc.fence()
        torch.cuda.synchronize()
        # (the launches after the one that left the residue first: what they return must not depend on it)
        for i, (at, n, o, r) in reversed(list(enumerate(runs))):
            o, r = o.cpu().numpy(), r.cpu().numpy()
            if i == 0:
                o, r, at, n = o[1:], r[1:], at + 1, n - 1
            _same(o, r, want[at:at + n], want_res[at:at + n], "codec %d seg %s lanes %d launch %d (%d frames)" % (codec, seg, lanes, i, n))
        assert enc.watchdog() == 1, (lanes, enc.watchdog())
        o, r = runs[0][2].cpu().numpy(), runs[0][3].cpu().numpy()
        assert r[0].tolist() == [RELEASED, 0, 0, 0] and not o[0].any(), (lanes, r[0].tolist())
        enc.close()
    # the one-frame workspace: the first call leaves the residue (and is encoded again by the host), the calls after it read the workspace
    enc = _ctx(codec, PSXHIP_MDEC_SPLIT_WITHHOLD="0:%s:1:1" % seg)
    for k in range(6):
        out, res = enc.encode_frames_host(fr[k:k + 1], BUDGET)
        _same(out, res, want[k:k + 1], want_res[k:k + 1], "codec %d seg %s one-frame call %d" % (codec, seg, k))
    o, r = enc.encode_frames_device(d[6:18], BUDGET)
    torch.cuda.synchronize()
    _same(o.cpu().numpy(), r.cpu().numpy(), want[6:18], want_res[6:18], "codec %d seg %s device after one-frame calls" % (codec, seg))
    assert enc.watchdog() == 1
    enc.close()


# ---- child processes: short patience, co-tenants

def _run_children(specs, timeout):
    """start every child (at most three at once), wait for all; a child that dies by a signal or times out fails the test"""
    assert len(specs) <= 3
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, **env),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for args, env in specs]
    outs = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=timeout)
            outs.append((p.returncode, so, se))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    reports = []
    for rc, so, se in outs:
        assert rc == 0, (rc, so[-800:], se[-2000:])
        reports.append(json.loads(so.strip().splitlines()[-1]))
    return reports


@pytest.mark.parametrize("patience", [1, 64, 4000])
def test_short_patience_host_exact_device_exact_or_released(patience):
    """PSXHIP_MDEC_SPLIT_PATIENCE: rendezvous that give up after a few ticks, so frames are released and their late groups publish
    into workspaces the next launch uses -- codecs 0 and 1, device launches of 1..12 frames and one-frame calls"""
    reps = _run_children([(["stress", "0", "24"], {"PSXHIP_MDEC_SPLIT_PATIENCE": str(patience)}),
                          (["stress", "1", "24"], {"PSXHIP_MDEC_SPLIT_PATIENCE": str(patience)})], timeout=600)
    for r in reps:
        assert r["host_mismatch"] == 0 and r["device_mismatch"] == 0, r
        assert r["lost"] == r["device_released"] + r["host_released"], r
    if patience == 1:
        assert all(r["lost"] > 0 for r in reps), reps


@pytest.mark.parametrize("tenants", [2, 3])
def test_cotenant_processes_on_one_gpu(tenants):
    """two, then three processes on one GPU, each one-frame calls and 12-frame device launches at the default patience: no frame
    differs from the oracle (a device frame may be released when a neighbour holds the CUs; each process says how many)"""
    reps = _run_children([(["stress", str(i % 3), "60"], {}) for i in range(tenants)], timeout=600)
    for r in reps:
        assert r["host_mismatch"] == 0 and r["device_mismatch"] == 0, r
    print("lost per tenant:", [r["lost"] for r in reps])


def _child_stress(codec, iterations):
    import torch
    from psxavenc_amd.mdec import MdecEncoder
    fr = _frames(24, 60 + codec, amp=7)
    want, want_res, rc = O.mdec_encode(codec, W, H, fr, BUDGET)
    assert rc == 0
    enc = MdecEncoder(codec, W, H, max_frame_size=BUDGET, device=0)
    d = torch.from_numpy(fr).to("cuda:0")
    rep = dict(codec=codec, host_mismatch=0, device_mismatch=0, device_released=0, host_released=0, frames=0)
    sizes = (1, 12, 3, 7, 1, 2, 12, 5, 1, 9, 4, 11)
    host_before = enc.watchdog()
    for it in range(iterations):
        n = sizes[it % len(sizes)]
        at = (it * 5) % (24 - n + 1)
        o, r = enc.encode_frames_device(d[at:at + n], BUDGET)
        torch.cuda.synchronize()
        o, r = o.cpu().numpy(), r.cpu().numpy()
        for k in range(n):
            if r[k, 0] == RELEASED:
                rep["device_released"] += 1
                if r[k, 1:].any() or o[k].any():
                    rep["device_mismatch"] += 1
            elif not (np.array_equal(r[k], want_res[at + k]) and np.array_equal(o[k, :BUDGET], want[at + k])):
                rep["device_mismatch"] += 1
        rep["frames"] += n
        k = (it * 7) % 24
        before = enc.watchdog()
        out, res = enc.encode_frames_host(fr[k:k + 1], BUDGET)
        rep["host_released"] += enc.watchdog() - before
        if not (np.array_equal(res[0], want_res[k]) and np.array_equal(out[0], want[k])):
            rep["host_mismatch"] += 1
    rep["lost"] = enc.watchdog() - host_before
    enc.close()
    print(json.dumps(rep))


if __name__ == "__main__":
    if sys.argv[1] == "stress":
        _child_stress(int(sys.argv[2]), int(sys.argv[3]))
