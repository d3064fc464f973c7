"""Host-only checks of the device-RNG energised pore over shards (include/argonmc_shard.h): the order in which
``ShardedTemperatureSimulation.run`` issues the phases, with nothing that waits for the host inside the loop; the exact
sum of the ranks' 128-bit surface totals; the constructor without a seed; header, bindings and exports of the new entry
points.  The engine and the communicator are recording stand-ins handed in through ``engine=`` / ``comm=``: no context is
built.  (tests/test_gpu_dist_device_rng.py compares the real thing with the single context.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from argon_monte_carlo_amd import _lib, fields as FL, params as PR, surface as SU
from argon_monte_carlo_amd.dist import ShardedSimulation, ShardedTemperatureSimulation, _GlobalWallHooks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1000
STATS = dict(n_pp=1, n_wall=2, n_oob_walls=0, n_oob_pp=0, n_paths=3, n_fp_errors=0, n_candidates=4)


class RecordingEngine:
    """Every call by name (and what matters of its arguments) into the shared log."""

    def __init__(self, log, surface=None, params=None):
        self.log, self._surface = log, surface
        self.surface_grid = None if params is None else SU.default_grid(params)

    def __getattr__(self, name):                # temp_begin, temp_cases_device, mg_hits_pack, mg_bounds, mg_pack, mg_sweep, ...
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a: self.log.append((name,) + tuple(v for v in a if isinstance(v, (int, bool))))

    def hits_buffers(self, world):
        return "hits_send", "hits_recv"

    def exchange_buffers(self, world):
        return "kin_send", "kin_recv"

    def candidate_buffers(self, world):
        return "cand_send", "cand_recv"

    def mg_finish(self, want_stats=True):
        self.log.append(("mg_finish", bool(want_stats)))
        return dict(STATS) if want_stats else None

    def shard_run_end(self, nsteps):
        self.log.append(("shard_run_end", nsteps))
        return dict(STATS), np.arange(3.0 * nsteps).reshape(nsteps, 3), np.ones((nsteps, 3), dtype=bool)

    def surface_read(self):
        self.log.append(("surface_read",))
        return self._surface


class RecordingComm:
    shortcut = True

    def __init__(self, log, reduce=None):
        self.log, self.reduce = log, reduce

    def allgather_packed(self, send, recv):
        self.log.append(("allgather", send))

    def allgather_var(self, rows):
        self.log.append(("allgather_var",))
        raise AssertionError("allgather_var in the device-RNG mode")

    def allreduce_sum_ints(self, values):
        self.log.append(("allreduce", len(values)))
        return list(values) if self.reduce is None else self.reduce(list(values))


def _sim(world, rank=0, log=None, **kw):
    p, c = PR.pore_params(n=N, energised=True)
    log = [] if log is None else log
    eng = RecordingEngine(log, params=p, **kw.pop("engine_kw", {}))
    sim = ShardedTemperatureSimulation(p, rank, world, backend="gloo", engine=eng, comm=kw.pop("comm", None) or RecordingComm(log),
                                       consts=c, **kw)
    return sim, log, c


STEP_REPLICATED = ["temp_begin", "temp_cases_device", "mg_hits_pack", "allgather:hits_send", "mg_hits_sums", "mg_bounds",
                   "mg_pack", "allgather:kin_send", "mg_sweep", "mg_finish"]
STEP_BY_INDEX = STEP_REPLICATED[:8] + ["mg_detect", "allgather:cand_send", "mg_resolve", "mg_finish"]
HOST_SYNCS = ("allreduce", "allgather_var", "shard_run_end", "surface_read", "synchronize", "histograms", "download")


@pytest.mark.parametrize("replicated", [True, False])
def test_run_issues_the_phases_in_order_and_nothing_waits_for_the_host_inside_the_loop(replicated):
    sim, log, c = _sim(2, device_rng_seed=5)
    sim.replicated_detect = replicated
    st, sums, had = sim.run(c["dt"], 3)
    names = [e[0] + (":" + e[1] if e[0] == "allgather" else "") for e in log]
    step = STEP_REPLICATED if replicated else STEP_BY_INDEX
    assert names == ["shard_run_begin"] + step * 3 + ["shard_run_end", "allreduce"], names
    assert log[0] == ("shard_run_begin", 3)
    assert [e for e in log if e[0] == "mg_hits_sums"] == [("mg_hits_sums", 2, k) for k in range(3)]       # (world, row)
    assert [e for e in log if e[0] == "mg_finish"] == [("mg_finish", False)] * 3                            # no counter read-back
    last_finish = max(k for k, e in enumerate(log) if e[0] == "mg_finish")
    assert not [e for e in log[:last_finish + 1] if e[0] in HOST_SYNCS], log
    assert sums.shape == (3, 3) and had.shape == (3, 3) and had.dtype == bool
    assert all(st[k] == STATS[k] for k in ShardedSimulation.SUM_KEYS)


def test_single_step_returns_the_tuple_of_the_single_context_call():
    sim, log, c = _sim(2, device_rng_seed=5)
    out = sim.temp_timestep_device(c["dt"])
    assert len(out) == 7 and out[1:4] == (0.0, 1.0, 2.0) and out[4:] == (True, True, True)
    assert all(isinstance(v, float) for v in out[1:4]) and all(isinstance(v, bool) for v in out[4:])
    assert [e[0] for e in log][:1] == ["shard_run_begin"] and log[0] == ("shard_run_begin", 1)


def test_a_failing_rank_makes_every_rank_of_the_run_fail():
    """rank 1's status arrives in the all-reduce: rank 0, whose own run ended well, raises from the same call."""
    sim, log, c = _sim(2, device_rng_seed=5, comm=None)
    sim.comm.reduce = lambda v: [v[0], v[1] - 4] + v[2:]
    with pytest.raises(_lib.ArgonMCError) as ei:
        sim.run(c["dt"], 1)
    assert ei.value.code == -4 and "rank 1" in str(ei.value)


# ---- surface(): the ranks' 128-bit totals summed as 32-bit limbs -----------------------------------------------------------------
def _crafted_totals(nb):
    """Python ints per (rank, case, bin, quantity): carries across 2^32 and 2^64, negative totals, sign changes."""
    a = np.zeros((2, 7, nb + 1, 3), dtype=object)
    a[...] = 0
    pairs = [(2 ** 32 - 1, 1), (2 ** 64 - 1, 1), (-5, 3), (-(2 ** 64), 2 ** 64 - 1), (2 ** 96 + 2 ** 63, 2 ** 63), (-1, -(2 ** 32)),
             (-(2 ** 100) - 7, 2 ** 100), (123456789, 987654321), (-(2 ** 31), -(2 ** 31)), (2 ** 64 + 2 ** 32, -(2 ** 32) - 1)]
    for k, (u, v) in enumerate(pairs):          # (the large ones in dp_z and dE: derive() keeps the counts in int64)
        a[0, k % 7, k % (nb + 1), 1 + k % 2], a[1, k % 7, k % (nb + 1), 1 + k % 2] = u, v
    a[0, 0, 0, 0], a[1, 0, 0, 0] = 2 ** 32 - 1, 1
    a[0, 6, nb, 0], a[1, 6, nb, 0] = 2 ** 40 + 5, 2 ** 32 - 5
    rng = np.random.default_rng(8)
    for _ in range(40):
        s, b, q = int(rng.integers(7)), int(rng.integers(nb + 1)), int(rng.integers(1, 3))
        a[0, s, b, q] += int(rng.integers(-2 ** 62, 2 ** 62)) * int(rng.integers(1, 2 ** 40))
        a[1, s, b, q] += int(rng.integers(-2 ** 62, 2 ** 62)) * int(rng.integers(1, 2 ** 40))
    return a


def test_surface_sums_the_ranks_limbs_exactly():
    p, _ = PR.pore_params(n=N, energised=True)
    nb = int(SU.default_grid(p).nbins)
    ints = _crafted_totals(nb)
    nf = np.array([[1, 0, 2 ** 40, 0, 0, 5, 0], [0, 3, 2 ** 40, 0, 0, 0, 7]], dtype=np.int64)
    flats, sims = [], []
    for rank in range(2):
        words = FL.ints_to_words(ints[rank])
        assert np.array_equal(FL.words_to_ints(words), ints[rank])
        sim, log, c = _sim(2, rank=rank, device_rng_seed=5, engine_kw=dict(surface=(words, nf[rank], 6)))
        sim.comm.reduce = lambda v: flats.append(v) or v
        sim.surface()
        sims.append(sim)
    assert len(flats) == 2 and len(flats[0]) == len(flats[1]) == 2 + 7 * (nb + 1) * 3 * 4 + 7
    assert all(abs(v) < 2 ** 32 for f in flats for v in f[2:-7])            # limbs: a sum over ranks cannot overflow int64
    for sim in sims:
        sim.comm.reduce = lambda v: [x + y for x, y in zip(*flats)]
        d = sim.surface()
        assert np.array_equal(FL.words_to_ints(np.asarray(d["totals"])), ints[0] + ints[1])
        assert np.array_equal(np.asarray(d["n_failed"]), nf[0] + nf[1]) and d["n_steps"] == 6


def test_surface_fails_on_every_rank_when_one_rank_fails():
    p, _ = PR.pore_params(n=N, energised=True)
    nb = int(SU.default_grid(p).nbins)
    words = np.zeros((7, nb + 1, 3, 2), dtype=np.int64)
    sim, log, c = _sim(2, device_rng_seed=5, engine_kw=dict(surface=(words, np.zeros(7, dtype=np.int64), 1)))
    sim.comm.reduce = lambda v: [v[0], v[1] - 6] + v[2:]
    with pytest.raises(_lib.ArgonMCError) as ei:
        sim.surface()
    assert ei.value.code == -6 and "rank 1" in str(ei.value)


# ---- without a seed ------------------------------------------------------------------------------------------------------------------
def test_without_a_seed_the_object_is_the_hand_over_driver_of_before():
    sim, log, c = _sim(2)
    assert sim._device_rng is None and isinstance(sim._hooks, _GlobalWallHooks) and sim._hooks.e is sim.engine
    assert (sim.lo, sim.hi, sim.n, sim.replicated_detect) == (0, N // 2, N, True)
    with pytest.raises(ValueError):
        sim.temp_timestep_device(c["dt"])
    with pytest.raises(ValueError):
        sim.enable_surface()
    st = sim.run(c["dt"], 2)                    # ShardedSimulation.run: the loop of timesteps, counters read at the last one
    names = [e[0] for e in log]
    assert names == ["mg_local", "mg_pack", "allgather", "mg_sweep", "mg_finish"] * 2 + ["allreduce"], names
    assert [e for e in log if e[0] == "mg_finish"] == [("mg_finish", False), ("mg_finish", True)] and st["n_pp"] == STATS["n_pp"]


# ---- header and bindings -----------------------------------------------------------------------------------------------------------
def test_shard_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "argonmc_shard.h")).read()
    declared = {}
    for m in re.finditer(r"^int (amc_[a-z_]+)\(([^;]*)\);", hdr, flags=re.M):
        declared[m.group(1)] = [a for a in m.group(2).split(",") if a.strip()]
    assert set(declared) == set(_lib.SHARD_SIGNATURES) and len(declared) == 5, set(declared) ^ set(_lib.SHARD_SIGNATURES)
    assert not set(_lib.SHARD_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name, args in declared.items():
        res, argtypes = _lib.SHARD_SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(args), (name, args, argtypes)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes, name
    assert '#include "argonmc_shard.h"' in open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert os.path.join(ROOT, "include", "argonmc_shard.h") in _lib._source_files()


@pytest.mark.parametrize("lang,std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_header_with_the_shard_entry_points_compiles_as_c_and_cxx(tmp_path, lang, std):
    cc = shutil.which("cc" if lang == "c" else "c++")
    if cc is None:
        pytest.skip("no host compiler")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "argonmc.h"\n'
                   "int (*view_)(amc_ctx *, int, void **, void **, int64_t *) = amc_mg_hits_view;\n"
                   "int (*pack_)(amc_ctx *, int) = amc_mg_hits_pack;\n"
                   "int (*sums_)(amc_ctx *, int, int64_t) = amc_mg_hits_sums;\n"
                   "int (*begin_)(amc_ctx *, int64_t) = amc_temp_shard_run_begin;\n"
                   "int (*end_)(amc_ctx *, int64_t, amc_step_stats *) = amc_temp_shard_run_end;\n")
    r = subprocess.run([cc, "-x", lang, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "t.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


PART_HEADERS = ["corr", "flux", "mfp", "vdf", "transit", "pair", "shard"]


@pytest.mark.parametrize("lang,std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_every_part_header_may_follow_the_main_header(tmp_path, lang, std):
    """argonmc.h includes its seven part headers; a caller who names one of them as well must not meet redefinitions."""
    cc = shutil.which("cc" if lang == "c" else "c++")
    if cc is None:
        pytest.skip("no host compiler")
    parts = sorted(f[len("argonmc_"):-2] for f in os.listdir(os.path.join(ROOT, "include")) if f.startswith("argonmc_") and f.endswith(".h"))
    assert parts == sorted(PART_HEADERS), parts
    for part in PART_HEADERS:
        src = tmp_path / ("t_%s.%s" % (part, "c" if lang == "c" else "cpp"))
        src.write_text('#include "argonmc.h"\n#include "argonmc_%s.h"\n#include "argonmc_%s.h"\n#include "argonmc.h"\n'
                       "int version_(void) { return AMC_ABI_VERSION; }\n" % (part, part))
        r = subprocess.run([cc, "-x", lang, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                            str(tmp_path / ("t_%s.o" % part))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, (part, r.stdout.decode())
