"""CPU only: amc_init_separate's HOST code under AddressSanitizer and UBSan over the stand-in HIP runtime of tests/host_san/
(hip_shim.cpp) — what the call refuses, the smallest systems without a launch, the six launches of one search, the
work space given back, and an allocation failure at every allocation of the call (amc_owned_count is the same before and after).

tests/host_san/ic_driver.cpp is a stand-alone program: it is linked with the library's .hip files compiled host-only, in a pytest
temporary directory; nothing of it is loaded into Python.  Kernels do not run there."""
import os
import re
import shutil
import subprocess
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


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout.decode(errors="replace")[-4000:]
    return r.stdout.decode(errors="replace")


def _build(out):
    hips = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    host = ["-O1", "-g", "-std=c++17", "-ffp-contract=off"] + SAN
    jobs = [[HIPCC] + host + ["--offload-arch=gfx950", "--offload-host-only", "-w", "-c", os.path.join(CSRC, f), "-o", os.path.join(out, f[:-4] + ".o")]
            for f in hips]
    inc = ["-I", os.path.join(ROOT, "include"), "-I", HERE, "-isystem", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]
    jobs += [[CLANGXX] + host + ["-Wall", "-Werror"] + inc + ["-c", os.path.join(HERE, f), "-o", os.path.join(out, f[:-4] + ".o")]
             for f in ("hip_shim.cpp", "ic_driver.cpp")]
    with ThreadPoolExecutor(max_workers=min(JOBS, os.cpu_count() or 1)) as pool:
        list(pool.map(_run, jobs))
    objs = [os.path.join(out, f[:-4] + ".o") for f in hips]
    # a host-only compile leaves the file's device code object undefined (__hip_fatbin_<hash>): define each, and nothing else
    nm_tool = shutil.which("nm") or shutil.which("llvm-nm")
    nm = _run([nm_tool, "-u"] + objs) if nm_tool else "\n".join(
        ln for ln in _run([os.path.join(ROCM, "llvm", "bin", "llvm-readelf"), "-s", "-W"] + objs).splitlines() if " UND " in ln)
    fatbins = sorted(set(re.findall(r"\b(__hip_fatbin_[0-9a-f]+)\b", nm)))
    assert fatbins
    stub = os.path.join(out, "fatbins.c")
    with open(stub, "w") as fh:
        fh.write("".join("const char %s[8] = {0};\n" % s for s in fatbins))
    exe = os.path.join(out, "ic_driver")
    _run([CLANGXX] + SAN + ["-x", "c", stub, "-x", "none"] + objs + [os.path.join(out, "hip_shim.o"), os.path.join(out, "ic_driver.o"), "-lm", "-o", exe])
    return exe


def test_host_side_runs_clean_under_the_sanitizers(tmp_path):
    exe = _build(str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    env.pop("AMC_IC_CELLS", None)
    r = subprocess.run(["timeout", "-k", "5", "100", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=str(tmp_path))
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    print(out + err[-6000:])
    assert not re.search(r"Sanitizer|runtime error", err), err[-6000:]
    assert r.returncode == 0, (r.returncode, err[-6000:])
    assert "ic_separate: ok" in out
    m = re.search(r"A = (\d+) allocations, every k = 1 \.\. (\d+) failed once", out)
    assert m and int(m.group(1)) == int(m.group(2)) == 9, out
