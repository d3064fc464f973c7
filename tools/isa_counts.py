#!/usr/bin/env python3
"""Instruction and register counts per kernel of one HIP source file of argon_monte_carlo_amd/csrc.

    python tools/isa_counts.py amc_clusters.hip [--filter k_clusters_wide] [--keep-asm out.s]

Compiles the file to gfx950 assembly with the Makefile's own flags (device side only) and prints one JSON object:
kernel symbol -> {demangled, instructions, flat, global, ds, waitcnt: {form: count}, vgprs, sgpr_spill, vgpr_spill,
scratch_bytes}.  `flat` / `global` / `ds` count the instructions whose mnemonic starts with flat_ / global_ / ds_ — the
address space the compiler could prove for each access.  Register figures come from the code
object's metadata (what the loader reserves), not from the comments.
"""
import argparse
import collections
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "argon_monte_carlo_amd", "csrc")


def makefile_vars():
    """HIPCC, ARCH and CXXFLAGS as the Makefile sets them (environment overrides honoured like make's ?=)."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    v = {}
    for name in ("HIPCC", "ARCH", "CXXFLAGS"):
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
        v[name] = m.group(1).strip()
    for name in ("HIPCC", "ARCH"):
        v[name] = os.environ.get(name, v[name])
    v["CXXFLAGS"] = v["CXXFLAGS"].replace("$(ARCH)", v["ARCH"])
    return v


def hipcc_path():
    h = makefile_vars()["HIPCC"]
    return h if os.path.exists(h) else shutil.which("hipcc")


def compile_asm(src, out):
    v = makefile_vars()
    cmd = [hipcc_path()] + v["CXXFLAGS"].split() + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True, cwd=CSRC)


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(filt):
        filt = shutil.which("c++filt")
    if not filt:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(asm_text):
    # registers: the metadata note at the end of the file (one YAML map per kernel)
    # (vgpr_count is what the kernel occupies of the unified file: architectural VGPRs + AGPRs)
    meta = {}
    cur = None
    for line in asm_text.split("\n"):
        m = re.match(r"^  (- | {2})\.([a-z_]+):\s*(\S*)", line)      # keys of a kernel's own map sit at this depth only
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip("'\"")
        if m.group(2) == "symbol":
            val = cur["symbol"]
            meta[val[:-3] if val.endswith(".kd") else val] = cur
    res = {}
    body = None
    for line in asm_text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in meta:
            body = res[m.group(1)] = {"instructions": 0, "flat": 0, "global": 0, "ds": 0, "waitcnt": collections.Counter()}
            continue
        if line.startswith(".Lfunc_end"):
            body = None
            continue
        if body is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op = s.split()[0]
        body["instructions"] += 1
        for pre in ("flat", "global", "ds"):
            if op.startswith(pre + "_"):
                body[pre] += 1
        if op == "s_waitcnt":
            body["waitcnt"][" ".join(s.split()[1:])] += 1
    for sym, b in res.items():
        mt = meta[sym]
        b["waitcnt"] = dict(sorted(b["waitcnt"].items(), key=lambda kv: -kv[1]))
        b["vgprs"] = int(mt.get("vgpr_count", 0))
        b["agprs"] = int(mt.get("agpr_count", 0))
        b["sgpr_spill"] = int(mt.get("sgpr_spill_count", 0))
        b["vgpr_spill"] = int(mt.get("vgpr_spill_count", 0))
        b["scratch_bytes"] = int(mt.get("private_segment_fixed_size", 0))
    dm = demangle(list(res))
    for sym, b in res.items():
        b["demangled"] = dm[sym]
    return res


def counts(hip_file, keep_asm=None):
    src = hip_file if os.path.isabs(hip_file) else os.path.join(CSRC, os.path.basename(hip_file))
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        compile_asm(src, out)
        if keep_asm:
            shutil.copy(out, keep_asm)
        return parse(open(out).read())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("hip_file", help="a .hip file of argon_monte_carlo_amd/csrc")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--keep-asm", default=None, help="also copy the assembly to this path")
    a = ap.parse_args()
    res = counts(a.hip_file, a.keep_asm)
    res = {k: v for k, v in res.items() if a.filter in v["demangled"]}
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
