"""Building and running the lane programs (tests/cpu/*_lanes.cpp): a kernel file's own text compiled by g++ behind the stand-in
tests/cpu/hip_lanes/hip/hip_runtime.h and run lane by lane on the CPU -- under the host sanitizers in three lane orders, and once
more without them under gcov, which says which of the file's lines and template instantiations the records reached.

Test infrastructure only."""
import json
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "psxavenc_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
COVERAGE = ["-O0", "--coverage"]
ORDERS = (("ascending", 0), ("descending", 1), ("shuffled", 2))
SEED = 20240


def build(folder, name, flags):
    """tests/cpu/<name>.cpp -> folder/<name>, by way of folder/<name>.o (gcov's notes lie next to the object file)"""
    import pytest
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpu/%s.cpp" % name)
    obj, exe = os.path.join(str(folder), name + ".o"), os.path.join(str(folder), name)
    subprocess.run(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "tests/cpu/hip_lanes"), "-c", "-o", obj,
                    os.path.join(ROOT, "tests/cpu", name + ".cpp")], check=True)
    subprocess.run(["g++"] + flags + ["-o", exe, obj], check=True)
    return exe


# the one line ASan prints (once per process) when a program first switches ucontext fibers, as the wavefront model's programs do
# (tests/cpu/hip_lanes/hip_lanes_waves.h announces every switch to it with __sanitizer_start / finish_switch_fiber)
FIBER_WARNING = re.compile(r"\A==\d+==WARNING: ASan doesn't fully support makecontext/swapcontext functions and may produce false positives "
                           r"in some cases!\n")


def sanitizer_env():
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    return env


def own_stderr(text, fibers):
    """what a program wrote to stderr, without ASan's one line about fibers when the program runs the wavefront model"""
    return FIBER_WARNING.sub("", text, count=1) if fibers else text


def run(exe, src, dst, order=0, sanitized=True, fibers=False):
    """one child process in the caller's environment, the sanitizers' runtime linked in statically (as tests/test_ingest_core_cpu.py
    runs its program).  The sanitizer build must end with exit 0 and an empty stderr (`fibers`: but for FIBER_WARNING, once)"""
    env = sanitizer_env() if sanitized else dict(os.environ)
    p = subprocess.run([exe, src, dst, str(order), str(SEED)], capture_output=True, text=True, env=env, timeout=900)
    err = own_stderr(p.stderr, fibers and sanitized)
    assert p.returncode == 0 and not err.strip(), "%s, lane order %d, reported (exit %d):\n%s" % (
        os.path.basename(exe), order, p.returncode, err[-6000:])
    with open(dst, "rb") as f:
        return f.read()


def run_orders(exe, src, dst, fibers=False):
    """the output bytes, which every lane order must give alike"""
    outs = [(name, run(exe, src, dst, order, fibers=fibers)) for name, order in ORDERS]
    for name, got in outs[1:]:
        if got != outs[0][1]:
            first = next(i for i, (a, b) in enumerate(zip(got, outs[0][1])) if a != b) if len(got) == len(outs[0][1]) else -1
            raise AssertionError("%s: the %s lane order gives other bytes than the ascending one, the first at %d" % (os.path.basename(exe), name, first))
    return outs[0][1]


class Coverage:
    """what gcov says of one kernel file after the coverage build's runs: per line the largest count over the instantiations
    that hold it, and the functions with their lines and counts"""

    def __init__(self, folder, name, kernel_file):
        if not shutil.which("gcov"):
            import pytest
            pytest.fail("gcov is needed to read the coverage build's counts")
        p = subprocess.run(["gcov", "--json-format", "--stdout", "--demangled-names", name + ".gcda"], cwd=str(folder), capture_output=True,
                           text=True, check=True)
        report = json.loads(p.stdout)
        files = [f for f in report["files"] if os.path.basename(f["file"]) == kernel_file]
        assert len(files) == 1, [f["file"] for f in report["files"]]
        self.lines = {}
        for entry in files[0]["lines"]:
            self.lines[entry["line_number"]] = max(self.lines.get(entry["line_number"], 0), entry["count"])
        self.functions = [(f.get("demangled_name") or f["name"], f["start_line"], f["end_line"], f["execution_count"]) for f in files[0]["functions"]]
        with open(os.path.join(CSRC, kernel_file)) as f:
            self.text = f.read().split("\n")

    def instantiations(self, kernel):
        """{demangled name: count} of the instantiations of a __global__ template"""
        return {n: c for n, _, _, c in self.functions if re.search(r"\b%s<" % re.escape(kernel), n)}

    def unvisited(self):
        """[(line number, its text)] of the lines that hold code and never ran"""
        return [(n, self.text[n - 1].strip()) for n, c in sorted(self.lines.items()) if c == 0]

    def lines_of(self, names):
        """the line numbers inside the functions of these names"""
        inside = set()
        for n, start, end, _ in self.functions:
            if any(re.search(r"\b%s\b" % re.escape(x), n) for x in names):
                inside.update(range(start, end + 1))
        return inside
