"""The library's HOST code under AddressSanitizer and UBSan over a stand-in HIP runtime (tests/host_san/).

The twenty .hip files are compiled host-only with -fsanitize=address,undefined and linked with tests/host_san/hip_shim.cpp (no
HIP runtime) and tests/host_san/driver.cpp into ONE stand-alone program in a pytest temporary directory — never into the tree,
never into libargonmc.so, nothing of it is loaded into Python.  "Device" memory is a malloc block of exactly the size asked
for, filled with 0xA5; copies and memsets act on it at once; a launch runs nothing and is refused when a grid or block dimension
is zero.  So the scenarios see what the host enqueues — extents, ownership, error paths, read-backs of memory nobody cleared,
launch geometry — and nothing a kernel does.

Not driven, because they wait on the host for words only a kernel writes, or are plain host helpers without a context:
none of the former was met (amc_run's on-demand loop falls back on a stream synchronisation after 2 ms without progress);
amc_host_directions and amc_pairwise_cell are covered by tests/test_host.py and the GPU suite and are not driven here.
"""
import os
import re
import shutil
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "argon_monte_carlo_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "host_san")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
CLANGXX = os.path.join(ROCM, "llvm", "bin", "clang++")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
JOBS = 16

pytestmark = [
    pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(CLANGXX)), reason="no hipcc / ROCm clang++"),
    # sanitizer runs belong on a machine without a GPU
    pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU machine: the sanitized host build runs on CPU-only machines"),
]


def _run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, **kw)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout.decode(errors="replace")[-4000:]
    return r.stdout.decode(errors="replace")


def build_driver(out):
    """The sanitized program `out/driver`; returns (path, seconds the build took)."""
    t0 = time.time()
    hips = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert len(hips) >= 20, hips
    host = ["-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SAN
    jobs = [[HIPCC] + host + ["--offload-arch=gfx950", "--offload-host-only", "-w", "-c", os.path.join(CSRC, f), "-o",
             os.path.join(out, f[:-4] + ".o")] for f in hips]
    inc = ["-I", os.path.join(ROOT, "include"), "-I", HERE, "-isystem", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]
    jobs += [[CLANGXX] + host + ["-Wall", "-Werror"] + inc + ["-c", os.path.join(HERE, f), "-o", os.path.join(out, f[:-4] + ".o")]
             for f in ("hip_shim.cpp", "driver.cpp")]
    with ThreadPoolExecutor(max_workers=min(JOBS, os.cpu_count() or 1)) as pool:
        list(pool.map(_run, jobs))
    objs = [os.path.join(out, f[:-4] + ".o") for f in hips]
    # a host-only compile leaves the file's device code object undefined (__hip_fatbin_<hash>): define each, and nothing else
    nm_tool = shutil.which("nm") or shutil.which("llvm-nm")
    nm = _run([nm_tool, "-u"] + objs) if nm_tool else "\n".join(
        ln for ln in _run([os.path.join(ROCM, "llvm", "bin", "llvm-readelf"), "-s", "-W"] + objs).splitlines() if " UND " in ln)
    fatbins = sorted(set(re.findall(r"\b(__hip_fatbin_[0-9a-f]+)\b", nm)))
    assert fatbins, "no __hip_fatbin_ symbol is undefined: was this a host-only compile?"
    stub = os.path.join(out, "fatbins.c")
    with open(stub, "w") as fh:
        fh.write("".join("const char %s[8] = {0};\n" % s for s in fatbins))
    exe = os.path.join(out, "driver")
    _run([CLANGXX] + SAN + ["-x", "c", stub, "-x", "none"] + objs + [os.path.join(out, "hip_shim.o"), os.path.join(out, "driver.o"), "-lm", "-o", exe])
    return exe, time.time() - t0


@pytest.fixture(scope="session")
def driver(tmp_path_factory):
    exe, took = build_driver(str(tmp_path_factory.mktemp("host_san")))
    print("sanitized host build: %.1f s" % took)
    return exe


def run_scenario(exe, name, limit=100):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "5", str(limit), exe, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=os.path.dirname(exe))
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    print(out + err[-6000:] + "%s: %.1f s" % (name, time.time() - t0))
    return r.returncode, out, err


SCENARIOS = ["lifetime", "samplers", "sharded", "alloc_sweep", "empty_samplers"]


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario_runs_clean(driver, name):
    """lifetime: scenario 1 (and 4, the poison checks, which every scenario makes on what it reads); samplers: 2; sharded: 3;
    alloc_sweep: 5; empty_samplers: 6 (the launch log is examined at the end of every scenario)."""
    rc, out, err = run_scenario(driver, name)
    assert rc != 124 and rc != 137, "%s ran into its time limit: an entry point waits for a word only a kernel writes?" % name
    assert not re.search(r"Sanitizer|runtime error", err), err[-6000:]
    assert rc == 0, (rc, err[-6000:])
    assert ("%s: ok" % name) in out
    if name == "alloc_sweep":
        # every kind, the empty system too, and A printed for each
        assert len(re.findall(r"A = \d+ allocations, every k = 1 \.\. \d+ failed once", out)) == 8, out


def test_the_sanitizer_is_live_in_what_was_built(driver):
    """Scenario 7: an 8-byte overrun made by the driver itself through the stand-in's hipMemsetAsync must END the run."""
    rc, out, err = run_scenario(driver, "liveness")
    assert rc != 0 and "heap-buffer-overflow" in err, (rc, err[-3000:])
    assert "went unnoticed" not in out
