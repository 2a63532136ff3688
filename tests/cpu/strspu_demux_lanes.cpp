// tests/cpu/strspu_demux_lanes.cpp -- TEST INFRASTRUCTURE: runs the text of psxavenc_amd/csrc/strspu_demux_kernels.hip and of its host layer
// psxavenc_amd/csrc/psxhip_str_demux.cpp on the CPU under -fsanitize=address,undefined (tests/test_strspu_demux_lanes_cpu.py), behind the
// wavefront model of the stand-in tests/cpu/hip_lanes.  The program's text is tests/cpu/str_readers_lanes.inc, which says why the
// STR and the STRSPU reader share it.  A program, not a library.
#include "str_readers_lanes.inc"
