// tests/cpu/wave_probe_lanes.cpp -- TEST INFRASTRUCTURE: tests/cpu/wave_probe.hip behind the stand-in's wavefront model
// (tests/cpu/hip_lanes/hip_lanes_waves.h), for tests/test_wave_model_cpu.py.  The same text is built by hipcc for the MI355X in
// tests/test_gpu_wave_probe.py.  A program, not a library.
#define HIP_LANES_WAVES 1
#include "wave_probe.hip"
