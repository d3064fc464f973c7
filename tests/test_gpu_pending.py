"""GPU (-m gpu): every entry point behind every state a step can leave pending.

A step leaves two things for later (amc_ctx::step, csrc/amc_internal.h): `lazy_pending` — the sweep's results still sit in
the slot arrays and wait for the next streaming pass — and `commit_pending` — the sweep's commit (completed paths into the
histograms and records, the collision counters, the overlay) has not run.  Every entry point that reads or replaces state,
outputs or counters has to settle them first.  This module is the matrix of that rule:

  rows     PRODUCERS: ways to advance a context that end in each reachable combination of the two (amc_timestep; amc_run
           under its three plans; the stage calls, which leave nothing; one ShardEngine over the whole range, whose
           amc_mg_finish(ctx, NULL) leaves BOTH set in the cube; two ShardEngines in one process; the energised pore's
           host-handshake step, and amc_temp_run_device with a device seed)
  columns  CONSUMERS: the entry points, each called directly after the producer's last step.

Every cell compares with the oracle (`orc_mul`) stepped through the same steps, bit for bit: no tolerances.  All producers
advance the system by whole steps, so one oracle trajectory per system (geometry, N) serves every cell; a consumer that
changes the state (partial upload, reset) continues a copy of the oracle from that step.

Non-vacuity: at the top of every cell the ORACLE's last sweep before the consumer must have at least 3 p-p collisions and
at least one completed path (two engines: one owned by each rank) — otherwise a forgotten commit or a forgotten result would
change nothing.  The systems below start mid-flight (every particle has a collision behind it, `full_path_traveled` set,
path accumulators non-zero) with a raised cross-section, so that every collision of every sweep completes two paths; the
seeds and multipliers were chosen with the oracle on the CPU.

The energised rows.  Host handshake: the oracle runs its own host loop on random streams seeded like the device's.  Device
seed: a draw depends on (seed, particle, step, case, attempt) alone, so the oracle is led through the steps by a second
context stepped one amc_temp_begin / amc_temp_cases_device / amc_temp_end at a time, whose draws it replays case by case
and whose state it must reproduce bit for bit at every step (the pinning of
test_gpu_parity.test_device_rng_energised_walls_match_oracle_on_the_same_draws); the context under test runs
amc_temp_run_device and is compared with that oracle.
"""
import ctypes as C

import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime — the two-engine rows exchange through torch)

from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd._abi import AmcParams
from argon_monte_carlo_amd.dist import LocalRanks, shard_range

pytestmark = pytest.mark.gpu

SF = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"]
REC_KEY = ("step", "phase", "cell", "i", "j", "which")
REC_ALL = REC_KEY + ("total", "px", "py", "pz")
HIST_KEYS = ("total", "px", "py", "pz")


@pytest.fixture(scope="module")
def Engine():
    from argon_monte_carlo_amd.engine import Engine as E
    return E


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ---------------------------------------------------------------------------------------------- the systems and their oracle
# (geometry, N) -> cross-section multiplier (the knob of the existing high-collision tests), seed, time-step multiplier.
# The pore's own dt shrinks with the cross-section, and N = 20,000 is a few per cent of the reference's density: with the
# step 100 times longer the oracle has 25-45 p-p collisions and, from the fourth step on, 10-60 wall hits in every step
# (at the pore's own dt: none after the second step).
SYSTEMS = {("cube", 4096): (16.0, 41, 1.0), ("cube", 4097): (16.0, 41, 1.0), ("cube", 20_000): (16.0, 41, 1.0),
           ("pore", 20_000): (30.0, 41, 100.0)}


def make_system(kind, n):
    """(params, consts, the eleven initial arrays).  Positions and velocities are the synthetic initial conditions of the
    other GPU tests; the path accumulators describe particles mid-flight after an earlier collision."""
    mult, seed, _ = SYSTEMS[(kind, n)]
    sigma = 3.6e-19 * mult
    if kind == "cube":
        p, c = PR.cube_params_for_n(n, sigma=sigma)
        pos_vel = IC.cube_ic(p, c, seed=seed)
    else:
        p, c = PR.pore_params(n=n, sigma=sigma)
        pos_vel = IC.pore_ic(p, c, seed=seed)
    p.detect_mode = 1
    p.reserved1 = 1
    rng = np.random.default_rng(seed + n)
    span = float(p.hist_hi - p.hist_lo)
    # |(dx, dy, dz)| spread over 1.2 x the histogram range: most completed paths fall into bins, some beyond the last edge
    dxyz = rng.random((3, n)) * (1.2 * span / np.sqrt(3.0))
    d = np.sqrt((dxyz ** 2).sum(axis=0))
    init = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in pos_vel) + (d, dxyz[0].copy(), dxyz[1].copy(), dxyz[2].copy())
    return p, c, init, np.ones(n, dtype=np.uint8)


class Trajectory:
    """The oracle stepped once per system: state, prior positions, statistics and number of path records after every step."""

    def __init__(self, O, kind, n):
        self.O, self.kind, self.n = O, kind, n
        self.p, self.c, self.init, self.flag0 = make_system(kind, n)
        self.dt = self.c["dt"] * SYSTEMS[(kind, n)][2]
        self.orc = O.Oracle(self.p, mode="mul", path_capacity=1 << 20)
        self.orc.upload(*self.init, flag=self.flag0)
        self.states, self.priors, self.stats, self.npaths = [self.orc.state()], [None], [None], [0]

    def _advance(self):
        return self.orc.timestep(self.dt)

    def upto(self, k):
        while len(self.states) <= k:
            rc, st = self._advance()
            assert rc == 0
            self.states.append(self.orc.state())
            self.priors.append([self.orc.arr[a].copy() for a in ("px", "py", "pz")])
            self.stats.append(st)
            self.npaths.append(int(self.orc._sink.n))
        return self

    def state(self, k):
        return self.upto(k).states[k]

    def paths(self, k, since=0):
        """records of the steps [since, k), in the reference's append order"""
        self.upto(k)
        return self.orc.paths()[self.npaths[since]:self.npaths[k]]

    def fork(self, k, step=None):
        """a new oracle in the state after k steps (its records start empty; `step` is the key its next records carry)"""
        o = self.O.Oracle(self.p, mode="mul", path_capacity=1 << 18)
        st = self.state(k)
        o.upload(*[st[f] for f in SF], flag=st["flag"])
        o.step = k if step is None else step
        return o

    def assert_last_sweep_has_work(self, k, ranges):
        """the condition that keeps a cell from passing vacuously, on the oracle's own output"""
        self.upto(k)
        assert self.stats[k]["n_pp"] >= 3, (self.kind, self.n, k, self.stats[k])
        rec = self.paths(k, since=k - 1)
        rec = rec[rec["phase"] >= 16]                       # completed by the p-p sweep, not by a wall
        owner = np.where(rec["which"] == 0, rec["j"], rec["i"])
        for lo, hi in ranges:
            assert np.count_nonzero((owner >= lo) & (owner < hi)) >= 1, (self.kind, self.n, k, lo, hi)


# ---- the energised pore (N = 20,000, the specular pore's cross-section and lengthened step: 20-45 p-p collisions and 30-40
# energised wall hits per step in the oracle)
TEMP_SEED = 0x5EED2026


def make_temp_system(n):
    from argon_monte_carlo_amd.energised import SurfaceEnergies
    p, c = PR.pore_params(n=n, sigma=3.6e-19 * 30.0, energised=True)
    p.reserved0 |= 1
    p.reserved1 = 1
    init = IC.pore_ic(p, c, seed=41)
    rng = np.random.default_rng(41 + n)
    span = float(p.hist_hi - p.hist_lo)
    dxyz = rng.random((3, n)) * (1.2 * span / np.sqrt(3.0))
    full = tuple(init) + (np.sqrt((dxyz ** 2).sum(axis=0)), dxyz[0].copy(), dxyz[1].copy(), dxyz[2].copy())
    return p, c, full, np.ones(n, dtype=np.uint8), SurfaceEnergies(c)


def new_sampler(state=None):
    import random
    from argon_monte_carlo_amd.energised import DirectionSampler
    rs, py = np.random.RandomState(5), random.Random(5)
    if state is not None:
        rs.set_state(state[0])
        py.setstate(state[1])
    return DirectionSampler(rs, py)


def sampler_state(s):
    return s.np_rng.get_state(), s.py_rng.getstate()


class TempHostTrajectory(Trajectory):
    """The energised pore with the reference's host random streams: the oracle's own host loop."""

    def __init__(self, O, kind, n):
        self.O, self.kind, self.n = O, kind, n
        self.p, self.c, self.init, self.flag0, self.energies = make_temp_system(n)
        self.dt = self.c["dt"] * 100.0
        self.orc = O.Oracle(self.p, mode="mul", path_capacity=1 << 18)
        self.orc.upload(*self.init, flag=self.flag0)
        self.sampler = new_sampler()
        self.rng = [sampler_state(self.sampler)]            # the streams' state after every step
        self.states, self.priors, self.stats, self.npaths = [self.orc.state()], [None], [None], [0]

    def _advance(self):
        rc, st = self.orc.temp_timestep(self.dt, self.sampler, self.energies)[:2]
        self.rng.append(sampler_state(self.sampler))
        return rc, st

    def fork(self, k, step=None):
        return _TempHostFork(self, k, step)


class _TempHostFork:
    def __init__(self, T, k, step):
        self.T = T
        self.orc = Trajectory.fork(T, k, step)
        self.sampler = new_sampler(T.rng[k])

    def upload(self, *a):
        self.orc.upload(*a)

    def timestep(self, dt):
        return self.orc.temp_timestep(dt, self.sampler, self.T.energies)[:2]

    def state(self):
        return self.orc.state()

    def paths(self):
        return self.orc.paths()


def replay_device_step(eng, orc, dt, cfg):
    """One device-seed step on `eng`, replayed in the oracle on the draws the device used; the oracle must land on the
    device's state bit for bit (that pins it).  Returns (rc, the oracle's statistics)."""
    from argon_monte_carlo_amd.energised import CASES
    before = len(orc.paths())
    st = eng.temp_timestep_device(dt, cfg)[0]
    orc._temp_wall_count = 0
    orc._temp_errs = 0
    orc.drift(dt, True)
    orc.temp_specular()
    for case in CASES:
        idx, nm, cz, ok = orc.wall_hits(case)
        didx, dn, dcz, ddir, dEs = eng.device_draws(case)
        assert np.array_equal(idx, didx) and np.array_equal(nm, dn) and np.array_equal(cz, dcz), ("replay", case)
        orc.wall_apply(case, ddir, dEs)
    orc.bounds(True)
    rc, npp, _ = orc.sweep()
    orc.bounds(True)
    orc.step += 1
    so = dict(n_pp=npp, n_wall=orc._temp_wall_count, n_paths=len(orc.paths()) - before)
    dev, ref = eng.download(), orc.state()
    assert st["n_pp"] == npp and all(np.array_equal(dev[f], ref[f]) for f in SF), ("replay", st, so)
    return rc, so


class TempRunTrajectory(Trajectory):
    """The energised pore with a device seed: the oracle led by a second context, one device-seed step at a time."""

    def __init__(self, O, kind, n):
        from argon_monte_carlo_amd.energised import device_rng_config
        from argon_monte_carlo_amd.engine import EnergisedEngine
        self.O, self.kind, self.n = O, kind, n
        self.p, self.c, self.init, self.flag0, self.energies = make_temp_system(n)
        self.p.E_cold, self.p.E_hot = self.energies.cold, self.energies.hot      # Temp:83-84, the coated walls' constants
        self.cfg = device_rng_config(self.c, TEMP_SEED)
        self.dt = self.c["dt"] * 100.0
        self.orc = O.Oracle(self.p, mode="mul", path_capacity=1 << 18)
        self.orc.upload(*self.init, flag=self.flag0)
        self.lead = EnergisedEngine(AmcParams.from_buffer_copy(self.p))
        self.lead.upload(*self.init, flag=self.flag0)
        self.states, self.priors, self.stats, self.npaths = [self.orc.state()], [None], [None], [0]

    def _advance(self):
        return replay_device_step(self.lead, self.orc, self.dt, self.cfg)

    def fork(self, k, step=None):
        return _TempRunFork(self, k, step)


class _TempRunFork:
    def __init__(self, T, k, step):
        from argon_monte_carlo_amd.engine import EnergisedEngine
        self.T = T
        self.orc = Trajectory.fork(T, k, step)
        st = T.state(k)
        self.lead = EnergisedEngine(AmcParams.from_buffer_copy(T.p))
        self.lead.upload(*[st[f] for f in SF], flag=st["flag"])
        self.lead.set_step(self.orc.step)                   # (the step word of the draws)

    def upload(self, *a):
        self.orc.upload(*a)
        self.lead.upload(*a)

    def timestep(self, dt):
        return replay_device_step(self.lead, self.orc, dt, self.T.cfg)

    def state(self):
        return self.orc.state()

    def paths(self):
        return self.orc.paths()


_TRAJ = {}
_TRAJ_CLASS = {"temp_host": TempHostTrajectory, "temp_run": TempRunTrajectory}


def trajectory(O, kind, n, prod=""):
    key = (prod if kind == "temp" else kind, n)
    if key not in _TRAJ:
        _TRAJ[key] = _TRAJ_CLASS.get(key[0], Trajectory)(O, kind, n)
    return _TRAJ[key]


# ---------------------------------------------------------------------------------------------- the producers
ENV_PLANS = ("AMC_ORDERED_ALWAYS", "AMC_OVERLAP", "AMC_OD_MAX_N", "AMC_OD_AHEAD", "AMC_MG_REPLICATED")
# name -> (environment at context creation, steps, engines)
PRODUCERS = {
    "timestep": ({}, 3, 1),
    "run_plain9": ({"AMC_ORDERED_ALWAYS": "1"}, 9, 1), "run_plain12": ({"AMC_ORDERED_ALWAYS": "1"}, 12, 1),
    "run_od9": ({}, 9, 1), "run_od12": ({}, 12, 1),
    "run_ovl9": ({"AMC_OVERLAP": "1"}, 9, 1), "run_ovl12": ({"AMC_OVERLAP": "1"}, 12, 1),
    "stages": ({}, 3, 1),
    "shard1": ({}, 3, 1),
    "shard2_rep": ({}, 3, 2), "shard2_idx": ({}, 3, 2),
    "temp_host": ({}, 3, 1),                # three host-handshake steps, each ending in amc_temp_end
    "temp_run": ({}, 3, 1),                 # amc_temp_run_device(dt, 3) with a device seed
}
# steps of "one more step of the same producer": what keeps a run producer on its plan (amc_run: the overlapped run from 2
# steps, the ordered workgroup on demand from AMC_OD_MIN_STEPS = 8)
MORE = {"run_od": 8, "run_ovl": 2}
SINGLE_SYSTEMS = [("cube", 4096), ("cube", 20_000), ("pore", 20_000)]
PAIR_SYSTEMS = [("cube", 4096), ("cube", 4097), ("cube", 20_000), ("pore", 20_000)]
CASES = [(prod, kind, n) for prod, (_, _, engines) in PRODUCERS.items()
         for kind, n in ([("temp", 20_000)] if prod.startswith("temp") else SINGLE_SYSTEMS if engines == 1 else PAIR_SYSTEMS)]
# what does not exist for the energised engine is no row at all: the stage calls, amc_run, the mg_* entry points without the
# handshake, pairwise_cell (a cell context's)


def case_id(case):
    return "%s-%s-%d" % case


def cases(skip=None):
    """the matrix's rows for one column; `skip` maps a producer-name prefix (or a geometry) to the one-line reason its cell
    does not exist"""
    out = []
    for case in CASES:
        why = next((r for pre, r in (skip or {}).items() if case[0].startswith(pre) or case[1] == pre), None)
        out.append(pytest.param(case, id=case_id(case), marks=[pytest.mark.skip(reason=why)] if why else []))
    return pytest.mark.parametrize("case", out)


class Rig:
    """One producer on one system: the context(s), and the oracle trajectory they have to follow."""

    def __init__(self, O, case, monkeypatch, keep_prior=False, fields=False):
        from argon_monte_carlo_amd.engine import EnergisedEngine, Engine, ShardEngine
        self.prod, self.kind, self.n = case
        env, self.steps, self.world = PRODUCERS[self.prod]
        for name in ENV_PLANS:
            monkeypatch.delenv(name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        self.T = trajectory(O, self.kind, self.n, self.prod)
        self.more = next((m for pre, m in MORE.items() if self.prod.startswith(pre)), 1)
        self.run_steps = 0                  # steps handed to amc_run
        self.dt = self.T.dt
        self.p = AmcParams.from_buffer_copy(self.T.p)
        if keep_prior:
            self.p.reserved0 |= 1
        self.k = 0                          # whole steps done
        self.home_stream = None             # the stream the contexts run on (None: their own)
        if self.prod.startswith("shard"):
            self.home_stream = torch.cuda.current_stream().cuda_stream
            self.ranges = [shard_range(self.n, r, self.world) for r in range(self.world)]
            self.engs = [ShardEngine(self.p, lo, hi) for lo, hi in self.ranges]
            for e in self.engs:
                e.set_stream(self.home_stream)          # (the exchange below is torch's: same stream)
        else:
            self.ranges = [(0, self.n)]
            self.engs = [EnergisedEngine(self.p) if self.kind == "temp" else Engine(self.p)]
        if self.prod == "temp_host":
            self.sampler = new_sampler()
        for e in self.engs:
            e.upload(*self.T.init, flag=self.T.flag0)
            if fields:
                e.fields_config(FL.default_grid(self.p))
        if self.prod.startswith("shard"):
            # (the exchange is the helper's copy on the contexts' one stream, in launch order: the same bytes a copy through
            # the host delivers — tools/rehearse_ranks.py compares that path with a single context bit for bit)
            self.job = LocalRanks(self.engs, replicated=self.prod != "shard2_idx")

    def close(self):
        for e in self.engs:
            e.close()

    # -- stepping ---------------------------------------------------------------------------------------------------------
    def _shard_step(self, want):
        sts = self.job.step(self.dt, want)
        if not want:
            return None
        return {"n_pp": sts[0]["n_pp"], "n_paths": sum(s["n_paths"] for s in sts)}

    def _stage_step(self):
        e = self.engs[0]
        e.stage_drift(self.dt)
        st = e.stage_walls()
        npaths = st["n_paths"]
        if self.kind == "pore":
            e.stage_bounds()
        st = e.stage_sweep()
        if self.kind == "pore":
            e.stage_bounds()
        return {"n_pp": st["n_pp"], "n_paths": npaths + st["n_paths"]}

    def assert_plan(self):
        """amc_run took the plan the row is named after (it falls back to the plain loop quietly).  Called when the cell is
        over: amc_overlap_stats reads the counters, which settles what the producer left."""
        if not self.prod.startswith("run") or not self.run_steps:
            return
        s = self.engs[0].overlap_stats()
        if self.prod.startswith("run_ovl"):
            assert s["steps"] == self.run_steps and s["on_demand_steps"] == 0, (self.prod, s, self.run_steps)
        elif self.prod.startswith("run_od"):
            assert s["on_demand_steps"] >= self.run_steps and s["steps"] == 0, (self.prod, s, self.run_steps)
        else:
            assert s["steps"] == 0 and s["on_demand_steps"] == 0, (self.prod, s)

    def produce(self):
        """the producer's steps; the context is left as its last call leaves it"""
        e = self.engs[0]
        if self.prod == "timestep":
            for _ in range(self.steps):
                e.timestep(self.dt)
        elif self.prod.startswith("run"):
            e.run(self.dt, self.steps)
            self.run_steps += self.steps
        elif self.prod == "temp_host":
            for _ in range(self.steps):
                e.temp_timestep(self.dt, self.sampler, self.T.energies)
        elif self.prod == "temp_run":
            e.temp_run_device(self.dt, self.steps, self.T.cfg)
        elif self.prod == "stages":
            for _ in range(self.steps):
                self._stage_step()
        else:
            for _ in range(self.steps):
                self._shard_step(False)
        self.k += self.steps
        self.T.assert_last_sweep_has_work(self.k, self.ranges)
        return self

    def one_more(self):
        """one more step of the same producer — `self.more` steps in one call where the producer's plan needs as many;
        returns their n_pp and n_paths"""
        e = self.engs[0]
        if self.prod == "timestep":
            st = e.timestep(self.dt)
        elif self.prod.startswith("run"):
            st = e.run(self.dt, self.more)
            self.run_steps += self.more
        elif self.prod == "stages":
            st = self._stage_step()
        elif self.prod == "temp_host":
            st = e.temp_timestep(self.dt, self.sampler, self.T.energies)[0]
        elif self.prod == "temp_run":
            st = e.temp_run_device(self.dt, 1, self.T.cfg)[0]
        else:
            st = self._shard_step(True)
        self.k += self.more
        return {"n_pp": st["n_pp"], "n_paths": st["n_paths"]}

    def follow(self, orc):
        """the oracle `orc` through the steps of one_more(); their n_pp and n_paths"""
        tot = {"n_pp": 0, "n_paths": 0}
        for _ in range(self.more):
            rc, so = orc.timestep(self.dt)
            assert rc == 0
            tot = {f: tot[f] + so[f] for f in tot}
        return tot

    # -- the consumers, over all ranks --------------------------------------------------------------------------------------
    def download(self):
        """the state assembled from the owners (one engine: its download)"""
        parts = [e.download() for e in self.engs]
        return {f: np.concatenate([d[f][lo:hi] for d, (lo, hi) in zip(parts, self.ranges)]) for f in SF + ["flag"]}

    def histograms(self):
        res = [e.histograms() for e in self.engs]
        return sum(r[0].astype(np.int64) for r in res), sum(int(r[1]) for r in res)

    def paths_pending(self):
        tot = 0
        for e in self.engs:
            pend = C.c_size_t(0)
            e._ck(e.lib.amc_paths_pending(e._ctx, C.byref(pend)))
            tot += pend.value
        return tot

    def drain(self):
        rec = np.concatenate([e.drain_paths(sort=False) for e in self.engs])
        return rec[np.lexsort(tuple(rec[f] for f in reversed(REC_KEY)))]

    def upload(self, **arrays):
        for e in self.engs:
            e.upload(**arrays)

    def to_stream(self, ptr):
        for e in self.engs:
            if ptr is None:
                e._ck(e.lib.amc_set_stream(e._ctx, None))      # back to the context's own stream
            else:
                e.set_stream(ptr)

    # -- the comparisons ----------------------------------------------------------------------------------------------------
    def assert_state(self, ref, what):
        dev = self.download()
        for f in SF:
            assert np.array_equal(dev[f], ref[f]), (what, f, np.flatnonzero(dev[f] != ref[f])[:5])
        assert np.array_equal(dev["flag"].astype(bool), ref["flag"].astype(bool)), (what, "flag")
        return dev

    def assert_histograms(self, paths, what):
        counts, tot = self.histograms()
        p = self.p
        print(what, "device total", tot, "oracle paths", len(paths), "device in-range", counts.sum(axis=1))
        assert tot == len(paths), (what, tot, len(paths))
        for row, key in enumerate(HIST_KEYS):
            ref, _ = np.histogram(paths[key], bins=int(p.hist_bins), range=(p.hist_lo, p.hist_hi))
            assert np.array_equal(counts[row], ref.astype(np.int64)), (what, key, int(counts[row].sum()), int(ref.sum()))
            outside = np.count_nonzero((paths[key] < p.hist_lo) | (paths[key] > p.hist_hi))
            assert int(counts[row].sum()) == tot - outside, (what, key)
        return counts, tot

    def assert_records(self, rec, ref, what):
        """`rec` (sorted by the reference-order key) against the oracle's list: the same records, every key and value, in
        the same order.  The stage calls are the exception: they do not advance the step index (one step = four calls,
        include/argonmc.h), so their records all carry the step of the last amc_reset_outputs and are compared without that
        key, sorted by the others."""
        assert len(rec) == len(ref), (what, len(rec), len(ref))
        key = REC_ALL
        if self.prod == "stages":
            key = [f for f in REC_ALL if f != "step"]
            rec = rec[np.lexsort(tuple(rec[f] for f in reversed(key)))]
            ref = ref[np.lexsort(tuple(ref[f] for f in reversed(key)))]
        else:
            # (the oracle appends in the reference's order, which is the order of the key)
            order = np.lexsort(tuple(ref[f] for f in reversed(REC_KEY)))
            assert np.array_equal(order, np.arange(len(ref))), what
        for f in key:
            assert np.array_equal(rec[f], ref[f]), (what, f, rec[f][:8], ref[f][:8])


@pytest.fixture
def rig(O, monkeypatch):
    made = []

    def make(case, **kw):
        r = Rig(O, case, monkeypatch, **kw)
        made.append(r)
        return r
    yield make
    try:
        for r in made:
            r.assert_plan()
    finally:
        for r in made:
            r.close()


# ---------------------------------------------------------------------------------------------- the columns
@cases()
def test_download(rig, case):
    r = rig(case).produce()
    r.assert_state(r.T.state(r.k), "download")


@cases()
def test_histograms(rig, case):
    r = rig(case).produce()
    r.assert_histograms(r.T.paths(r.k), "histograms")


@cases()
def test_paths_pending_then_drain(rig, case):
    r = rig(case).produce()
    ref = r.T.paths(r.k)
    assert r.paths_pending() == len(ref)
    r.assert_records(r.drain(), ref, "drain_paths")
    assert r.paths_pending() == 0


@cases()
def test_histograms_then_download(rig, case):
    r = rig(case).produce()
    r.assert_histograms(r.T.paths(r.k), "histograms first")
    r.assert_state(r.T.state(r.k), "download second")


@cases()
def test_download_then_histograms(rig, case):
    r = rig(case).produce()
    r.assert_state(r.T.state(r.k), "download first")
    r.assert_histograms(r.T.paths(r.k), "histograms second")


@pytest.mark.parametrize("reader", ["download", "histograms", "paths_pending"])
@cases()
def test_read_only_consumer_twice(rig, case, reader):
    r = rig(case).produce()
    if reader == "download":
        a = r.assert_state(r.T.state(r.k), "first download")
        b = r.assert_state(r.T.state(r.k), "second download")
        assert all(np.array_equal(a[f], b[f]) for f in a)
    elif reader == "histograms":
        a = r.assert_histograms(r.T.paths(r.k), "first histograms")
        b = r.assert_histograms(r.T.paths(r.k), "second histograms")
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    else:
        assert r.paths_pending() == r.paths_pending() == len(r.T.paths(r.k))


@cases()
def test_reset_outputs_then_one_more_step(rig, case):
    """amc_reset_outputs (include/argonmc.h): what was enqueued before it is discarded from the outputs, and its results
    still reach the particle arrays."""
    r = rig(case).produce()
    k = r.k
    for e in r.engs:
        e.reset_outputs()
    st = r.one_more()
    orc = r.T.fork(k, step=0)               # (the reset restarts the step index the records carry)
    so = r.follow(orc)
    r.assert_state(orc.state(), "state after reset + step")
    if r.prod != "temp_run":                # (the fork is the trajectory's next step; device draws depend on the step index)
        assert np.array_equal(orc.state()["x"], r.T.state(r.k)["x"])
    print("step after the reset: device", st, "oracle n_pp", so["n_pp"], "n_paths", so["n_paths"],
          "| the sweep before the reset had n_pp", r.T.stats[k]["n_pp"])
    assert st["n_pp"] == so["n_pp"], (st, so, "the sweep before the reset had", r.T.stats[k]["n_pp"])
    assert st["n_paths"] == so["n_paths"], (st, so)
    r.assert_histograms(orc.paths(), "histograms after reset + step")
    r.assert_records(r.drain(), orc.paths(), "records after reset + step")


@cases()
def test_partial_uploads_then_step(rig, case):
    r = rig(case).produce()
    k = r.k
    now = r.T.state(k)
    vel = {f: -now[f] for f in ("vx", "vy", "vz")}                          # every particle turned round
    pos = {f: np.roll(now[f], 1) for f in ("x", "y", "z")}                  # every particle at its neighbour's place
    orc = r.T.fork(k)
    r.upload(**vel)
    orc.upload(None, None, None, vel["vx"], vel["vy"], vel["vz"])
    r.upload(**pos)
    orc.upload(pos["x"], pos["y"], pos["z"], None, None, None)
    r.assert_state(orc.state(), "after the two partial uploads")
    r.one_more()
    r.follow(orc)
    r.assert_state(orc.state(), "a step after the partial uploads")
    # the paths of the producer's last sweep are in the outputs, followed by this step's
    r.assert_histograms(np.concatenate([r.T.paths(k), orc.paths()]), "histograms after the partial uploads")


@cases(skip={"run_od": "amc_run leaves the on-demand plan when a field grid is configured"})
def test_fields_sample_and_read(rig, case):
    from tests import fields_ref as REF
    r = rig(case, fields=True).produce()
    ref = r.T.state(r.k)
    for e, (lo, hi) in zip(r.engs, r.ranges):
        e.fields_sample()
        tot, ns, no = e.fields_read()
        sums, outside = REF.sample_state(e.field_grid, ref, lo, hi)
        assert ns == 1 and no == outside
        assert np.array_equal(tot, FL.ints_to_words(sums)), np.argwhere(tot != FL.ints_to_words(sums))[:5]
    r.assert_state(ref, "download after the sample")


@cases(skip={"cube": "prior_{x,y,z}_vals are the pore's (Pore:427-429): the cube keeps none",
             "run_od": "amc_run leaves the on-demand plan when prior positions are kept (reserved0 bit 0)",
             "run_ovl": "amc_run leaves the overlapped plan when prior positions are kept (reserved0 bit 0)"})
def test_download_prior(rig, case):
    r = rig(case, keep_prior=True).produce()
    ref = r.T.upto(r.k).priors[r.k]
    if r.kind == "pore":                    # (where the last step started from)
        assert all(np.array_equal(a, r.T.state(r.k - 1)[f]) for a, f in zip(ref, "xyz"))
    for e, (lo, hi) in zip(r.engs, r.ranges):
        got = e.download_prior()
        for a, b, f in zip(got, ref, "xyz"):
            assert np.array_equal(a[lo:hi], b[lo:hi]), ("prior", f)
    r.assert_state(r.T.state(r.k), "download after download_prior")


@cases(skip={"shard2": "the facade (sim.Simulation) drives one context",
             "temp": "TemperatureSimulation steps with random streams of its own: it cannot continue a context another producer "
                     "advanced (its checkpoint: test_gpu_parity.test_checkpoint_resume_continues_bit_identically)"})
def test_checkpoint_resume(rig, case, tmp_path):
    """save_checkpoint from the facade straight after the producer, load_checkpoint into a fresh context, more steps: the
    state, the completed-path lists and the histograms of an uninterrupted run."""
    from argon_monte_carlo_amd.sim import Simulation
    r = rig(case)
    more = 3
    a = Simulation(r.kind, params=r.p, consts=r.T.c, engine=r.engs[0])      # the facade on the producer's context
    r.produce()
    a.steps_done = r.k
    ck = str(tmp_path / "ck.npz")
    a.save_checkpoint(ck)
    b = Simulation(r.kind, params=AmcParams.from_buffer_copy(r.T.p), consts=r.T.c)
    try:
        b.load_checkpoint(ck)
        for _ in range(more):
            b.timestep(r.dt)
        end = r.k + more
        ref = r.T.state(end)
        dev = b.engine.download()
        for f in SF:
            assert np.array_equal(dev[f], ref[f]), ("resumed", f)
        assert np.array_equal(dev["flag"].astype(bool), ref["flag"].astype(bool))
        paths = r.T.paths(end)
        for name, key in (("completed_paths", "total"), ("completed_x_paths", "px"), ("completed_y_paths", "py"),
                          ("completed_z_paths", "pz")):
            got, want = np.array(getattr(b, name)), paths[key]
            if r.prod == "stages":          # (records of stage calls carry no step index: compared as a multiset)
                got, want = np.sort(got), np.sort(want)
            assert np.array_equal(got, want), ("resumed", name, len(got), len(want))
        counts = b.engine.histograms()[0].astype(np.int64) + b._hist_base.astype(np.int64)
        for row, key in enumerate(HIST_KEYS):
            want, _ = np.histogram(paths[key], bins=int(r.p.hist_bins), range=(r.p.hist_lo, r.p.hist_hi))
            assert np.array_equal(counts[row], want), ("resumed histogram", key, int(counts[row].sum()), int(want.sum()))
    finally:
        b.close()


@cases()
def test_set_stream_and_back_then_step(rig, case):
    r = rig(case).produce()
    second = torch.cuda.Stream()
    r.to_stream(second.cuda_stream)
    r.to_stream(r.home_stream)
    r.one_more()
    r.assert_state(r.T.state(r.k), "a step after set_stream there and back")
    r.assert_histograms(r.T.paths(r.k), "histograms after set_stream there and back")


@cases()
def test_init_synthetic_after_steps(rig, case, Engine):
    from argon_monte_carlo_amd.engine import EnergisedEngine
    r = rig(case).produce()
    cfg = IC.device_ic_config(r.p, r.T.c, 77, "cube" if r.kind == "cube" else "pore")
    for e in r.engs:
        e.init_synthetic(cfg)
    fresh = (EnergisedEngine if r.kind == "temp" else Engine)(AmcParams.from_buffer_copy(r.T.p))
    try:
        fresh.init_synthetic(cfg)
        want = fresh.download()
    finally:
        fresh.close()
    r.assert_state(want, "init_synthetic after steps")
    r.assert_histograms(r.T.paths(r.k), "histograms after init_synthetic")
    r.assert_records(r.drain(), r.T.paths(r.k), "records after init_synthetic")


@cases()
def test_measurement_calls_change_nothing(rig, case):
    r = rig(case).produce()
    for e in r.engs:
        e.overlap_stats()
        e.kernel_times()
        e.lists_stats()
    r.assert_histograms(r.T.paths(r.k), "histograms after overlap_stats / kernel_times / lists_stats")
    r.assert_state(r.T.state(r.k), "download after overlap_stats / kernel_times")
    for e in r.engs:
        e.overlap_stats()
        e.kernel_times()
        e.lists_stats()
    r.one_more()
    r.assert_state(r.T.state(r.k), "a step after overlap_stats / kernel_times")
    r.assert_records(r.drain(), r.T.paths(r.k), "records after overlap_stats / kernel_times")


# ---------------------------------------------------------------------------------------------- a producer of another kind next
@pytest.mark.parametrize("kind,n", SINGLE_SYSTEMS)
def test_hops_between_single_context_producers(O, monkeypatch, kind, n):
    """timestep -> run -> stage calls -> timestep on one context: the oracle's state after every hop."""
    r = Rig(O, ("timestep", kind, n), monkeypatch)
    try:
        e, T = r.engs[0], r.T
        e.timestep(r.dt); r.k += 1
        r.assert_state(T.state(r.k), "timestep")
        T.assert_last_sweep_has_work(r.k, r.ranges)
        e.run(r.dt, 9); r.k += 9
        r.assert_state(T.state(r.k), "timestep -> run")
        T.assert_last_sweep_has_work(r.k, r.ranges)
        r._stage_step(); r.k += 1
        r.assert_state(T.state(r.k), "run -> stage calls")
        T.assert_last_sweep_has_work(r.k, r.ranges)
        e.timestep(r.dt); r.k += 1
        r.assert_state(T.state(r.k), "stage calls -> timestep")
        T.assert_last_sweep_has_work(r.k, r.ranges)
        e.run(r.dt, 9); r.k += 9
        T.assert_last_sweep_has_work(r.k, r.ranges)
        e.timestep(r.dt); r.k += 1                                        # (no download in between)
        T.assert_last_sweep_has_work(r.k, r.ranges)
        r.assert_state(T.state(r.k), "run -> timestep")
        r.assert_histograms(T.paths(r.k), "histograms after the hops")
    finally:
        r.close()


@pytest.mark.parametrize("prod,kind,n", [("shard1", "cube", 4096), ("shard1", "pore", 20_000), ("shard2_rep", "cube", 4097),
                                         ("shard2_idx", "cube", 4097), ("shard2_rep", "pore", 20_000),
                                         ("shard2_idx", "pore", 20_000)])
def test_hops_sharded_step_download_sharded_step(O, monkeypatch, prod, kind, n):
    r = Rig(O, (prod, kind, n), monkeypatch)
    try:
        for hop in range(3):
            r._shard_step(False); r.k += 1
            r.T.assert_last_sweep_has_work(r.k, r.ranges)
            r.assert_state(r.T.state(r.k), ("sharded step, download", hop))
        r.assert_histograms(r.T.paths(r.k), "histograms after the hops")
    finally:
        r.close()
