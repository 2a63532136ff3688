#!/usr/bin/env python3
"""CPU study tool (uses the oracle, never the product): AC bits(scale) and the refinement lower bound of synthetic
frames, fed through the search-policy simulator (tests/cpu/search_sim.cpp).  The curve code is tests/mdec_hard_content.py's, which
tests/test_mdec_bound.py holds to the oracle; that test also runs the simulator on non-monotone frames."""
import ctypes as C
import os
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oracle_lib as O
from mdec_hard_content import curves, luts      # noqa: F401  (the one copy of the curve code)


if __name__ == "__main__":
    w, h, budget, amp, n = [int(x) for x in (sys.argv[1:6] if len(sys.argv) > 5 else [640, 480, 8192, 4, 8])]
    so = "/tmp/libsearch_sim.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests/cpu/search_sim.cpp")], check=True)
    L = C.CDLL(so)
    ip = C.POINTER(C.c_int)
    nblk = (w // 16) * (h // 16) * 6
    fixed = 12 * nblk + 10
    limit = 16 * ((budget - 8) // 2)
    fr = O.synth_frames(w, h, n, seed=1, amp=amp)
    for i in range(n):
        tb, df = curves(w, h, fr[i], range(1, 40))
        tb[40:] = tb[39]
        t = (tb + fixed).astype(np.int32)
        t[0] = 0
        f = (t - df).astype(np.int32)
        want = next((s for s in range(1, 64) if t[s] <= limit), 64)
        out = []
        for g in range(1, 24):
            npass, lo, hi = C.c_int(), C.c_int(), C.c_int()
            r = L.search_sim(t.ctypes.data_as(ip), f.ctypes.data_as(ip), limit, fixed, g, limit + 32 * nblk // 6, C.byref(npass), C.byref(lo), C.byref(hi))
            assert r == want, (r, want)
            out.append(npass.value)
        print("frame %d want %d  limit %d fixed %d  tb[want-2..want+1]=%s  passes by guess 1..23: %s" % (i, want, limit, fixed, t[max(1, want - 2):want + 2].tolist(), out))
