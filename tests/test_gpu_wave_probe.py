"""tests/cpu/wave_probe.hip on the MI355X: the same well-defined kernels the wavefront model runs on the CPU
(tests/test_wave_model_cpu.py), built by hipcc for gfx950 into a stand-alone program and run once as a fresh child process, against
the same plain-numpy answers (tests/wave_probe_ref.py), byte for byte.  The stand-in's reading of the shuffles' edges, of the DPP
controls with their row and bank masks and bound_ctrl, of mbcnt and of the bit-count functions at zero is thereby the hardware's:
without this the model could be wrong in the same way as the code it checks.  Only wave_probe.hip is built here; the deliberately
wrong kernels of tests/cpu/wave_wrong_lanes.cpp never reach a device."""
import os
import shutil
import subprocess

import pytest

import wave_probe_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_probe_on_the_device_gives_numpy_bytes(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, src, dst = str(tmp_path / "wave_probe"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests/cpu/wave_probe.hip")], check=True,
                   timeout=300)
    inputs = R.make_input()
    with open(src, "wb") as f:
        f.write(R.to_bytes(*inputs))
    want = R.expected(*inputs)
    p = subprocess.run(["timeout", "-k", "10", "60", exe, src, dst], capture_output=True, text=True)
    assert p.returncode == 0, "wave_probe ended with %d:\n%s" % (p.returncode, p.stderr[-4000:])
    with open(dst, "rb") as f:
        got = f.read()
    assert got == want, R.describe(got, want, inputs[0], inputs[2], inputs[3])
