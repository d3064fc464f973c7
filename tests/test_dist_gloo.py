"""world_size-2 (and 3) gloo test (CPU) of the multi-GPU driver argon_monte_carlo_amd.dist.ShardedSimulation.

The driver is exercised with a NumPy engine that implements the mg_* protocol with simple deterministic rules (not the
physics — that is tested on the GPU against the oracle).  What a rank does not own and has not received is poisoned with
NaN (the path accumulators of other ranks' particles always, their positions and velocities until the all-gather of the
step has delivered them), so a wrong shard range, a wrong block of the packed exchange, a stale velocity or a use of
owner-only state shows up as a difference from the single-process run of the same engine; -0.0 must survive too."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd._lib import ArgonMCError
from argon_monte_carlo_amd.dist import ShardedSimulation, TorchComm, shard_range
from tests.test_gpu_dist import _assert_same_error, _outcome, _run_ranks_outcomes

KEYS = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"]


class NumpyShardEngine:
    def __init__(self, n, lo, hi, cr):
        self.n, self.lo, self.hi, self.cr = n, lo, hi, cr
        self.a = {k: np.zeros(n) for k in KEYS}
        self.flag = np.zeros(n, dtype=np.uint8)
        self.own = np.zeros(n, dtype=bool)
        self.own[lo:hi] = True
        self.ncand = 0

    # -- Engine surface used by the driver
    def upload(self, x, y, z, vx, vy, vz, d=None, dx=None, dy=None, dz=None, flag=None):
        for k, v in zip(KEYS, [x, y, z, vx, vy, vz, d, dx, dy, dz]):
            if v is not None:
                self.a[k][:] = v
        for k in KEYS[6:]:
            self.a[k][~self.own] = np.nan         # accumulators of other ranks' particles are NEVER available locally

    def download(self):
        out = {k: v.copy() for k, v in self.a.items()}
        out["flag"] = self.flag.copy()
        return out

    def exchange_buffers(self, world):
        self.m = (self.n + world - 1) // world
        self.send, self.recv = np.zeros(6 * self.m), np.zeros(world * 6 * self.m)
        return torch.from_numpy(self.send), torch.from_numpy(self.recv)

    def mg_local(self, dt):
        s = slice(self.lo, self.hi)
        for p, v in zip("xyz", ("vx", "vy", "vz")):
            self.a[p][s] += dt * self.a[v][s]
        self.a["d"][s] += 1.0
        for k in KEYS[:6]:
            self.a[k][~self.own] = np.nan         # stale until this step's all-gather delivers them

    def mg_pack(self, world):
        t = self.send.reshape(6, self.m)
        t[:] = 0.0
        for e, k in enumerate(KEYS[:6]):
            t[e, :self.hi - self.lo] = self.a[k][self.lo:self.hi]

    def candidate_buffers(self, world):
        self.ccap = 4 * self.n
        self.csend = np.zeros(2 + 2 * self.ccap, dtype=np.int32)
        self.crecv = np.zeros(world * (2 + 2 * self.ccap), dtype=np.int32)
        return torch.from_numpy(self.csend), torch.from_numpy(self.crecv)

    def _unpack(self, world, rank):
        if world > 1:
            for r in range(world):
                lo, hi = shard_range(self.n, r, world)
                if r == rank:
                    assert (lo, hi) == (self.lo, self.hi)
                    continue
                blk = self.recv[r * 6 * self.m:(r + 1) * 6 * self.m].reshape(6, self.m)
                for e, k in enumerate(KEYS[:6]):
                    self.a[k][lo:hi] = blk[e, :hi - lo]

    def mg_detect(self, world, rank):
        """detection sharded by index: my particles against everybody, pairs with the lower-indexed partner kept"""
        self._unpack(world, rank)
        P = np.stack([self.a[k] for k in "xyz"], 1)
        assert not np.isnan(P).any()
        d2 = ((P[self.lo:self.hi, None, :] - P[None, :, :]) ** 2).sum(-1)
        i, j = np.nonzero(d2 < self.cr ** 2)
        i = i + self.lo
        keep = j < i
        i, j = i[keep], j[keep]
        perm = np.random.default_rng(rank).permutation(len(i))         # (the device finds them in no particular order)
        self.csend[:] = -7
        self.csend[0] = len(i)
        self.csend[2:2 + 2 * len(i):2] = i[perm]
        self.csend[3:3 + 2 * len(i):2] = j[perm]

    def mg_resolve(self, world):
        blk = 2 + 2 * self.ccap
        pairs = []
        for r in range(world):
            b = self.crecv[r * blk:(r + 1) * blk]
            k = int(b[0])
            pairs.append(np.stack([b[2:2 + 2 * k:2], b[3:3 + 2 * k:2]], 1))
        pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), dtype=np.int32)
        self._collide(pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64))

    def mg_sweep(self, world, rank):
        self._unpack(world, rank)
        P = np.stack([self.a[k] for k in "xyz"], 1)
        assert not np.isnan(P).any()
        d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)
        i, j = np.nonzero(np.tril(d2 < self.cr ** 2, -1))
        self._collide(i, j)

    def _collide(self, i, j):
        order = np.lexsort((j, i))
        self.ncand = len(order)
        v = {k: self.a[k] for k in ("vx", "vy", "vz")}
        for i, j in zip(i[order], j[order]):
            for k in v:                               # "collision": exchange velocities (both particles' velocities needed)
                v[k][i], v[k][j] = v[k][j], v[k][i]
            m = int((7 * int(i) + 3 * int(j)) % self.n)   # a third particle's velocity enters, wherever it lives
            if m != i and m != j:
                v["vx"][i] = v["vx"][i] + v["vx"][m] * 0.5
            for q in (i, j):                          # bookkeeping of a particle: its owner only
                if self.own[q]:
                    self.a["dx"][q] += abs(v["vx"][q])
                    self.flag[q] = 1
        assert not any(np.isnan(v[k]).any() for k in v)
        assert not any(np.isnan(self.a[k][self.own]).any() for k in KEYS)

    # -- energised-wall hooks (fake rules; the point is the global ordering of hits and of the RNG draws)
    def temp_begin(self, dt):
        self.mg_local(dt)
        self.step = getattr(self, "step", 0) + 1

    def wall_hits(self, case):
        own = np.arange(self.lo, self.hi)
        hit = own[(own * 7 + case * 3 + self.step) % 11 == 0]
        nm = np.zeros((len(hit), 3))
        nm[:, case % 3] = 1.0 if case % 2 else -1.0
        ok = (hit % 5) != 0                                        # some contact solves "fail": no RNG draw for them
        self._hit = hit
        return hit.astype(np.int32), nm, self.a["z"][hit].copy(), ok

    def wall_apply(self, case, dirs, Es):
        hit = self._hit
        assert len(dirs) == len(hit) == len(Es)
        sp = np.sqrt(self.a["vx"][hit] ** 2 + self.a["vy"][hit] ** 2 + self.a["vz"][hit] ** 2)
        assert not np.isnan(sp).any()
        old_vz = self.a["vz"][hit].copy()
        for k, v in enumerate(("vx", "vy", "vz")):
            self.a[v][hit] = np.asarray(dirs)[:, k] * sp
        return old_vz - self.a["vz"][hit], np.asarray(Es) * sp

    def mg_bounds(self):
        pass

    def mg_finish(self, want_stats=True):
        return dict(n_pp=self.ncand if self.lo == 0 else 0, n_wall=self.hi - self.lo, n_oob_walls=0, n_oob_pp=0,
                    n_paths=0, n_candidates=self.ncand, n_clusters=0, n_rounds=1, n_fp_errors=0, flags=0)

    # -- sampled fields (fake totals: the shard's particle count in bin 0).  As on the device, a sample that meets a velocity
    # component outside |c| < 2^14 stops the sampling, and fields_read raises on the rank that owns the particle
    def fields_config(self, grid):
        self.field_grid = grid
        self.fields_reset()

    def fields_reset(self):
        self.f_tot = np.zeros((FL.grid_bins(self.field_grid), 7, 2), dtype=np.int64)
        self.f_samples, self.f_bad = 0, -1

    def fields_sample(self):
        v = np.stack([self.a[k][self.lo:self.hi] for k in ("vx", "vy", "vz")])
        bad = np.flatnonzero(~(np.abs(v) < 2.0 ** 14).all(axis=0))
        if self.f_bad < 0 and len(bad):
            self.f_bad = self.lo + int(bad[0])
        if self.f_bad < 0:
            self.f_tot[0, 0, 0] += self.hi - self.lo
            self.f_samples += 1

    def fields_read(self):
        if self.f_bad >= 0:
            raise ArgonMCError(-4, f"amc_fields: particle {self.f_bad} has a velocity component outside |c| < 2^14 m/s (or NaN); "
                                   "sampling stopped until amc_fields_reset")
        return self.f_tot.copy(), self.f_samples, 0


def make_state(n, seed=5):
    rng = np.random.default_rng(seed)
    pos = rng.random((3, n)) * 4e-9
    vel = rng.normal(size=(3, n)) * 300.0
    vel[0, ::7] = -0.0                                  # the exchange must keep the sign of zero
    return [pos[0], pos[1], pos[2], vel[0], vel[1], vel[2]]


def run_sim(n, rank, world, steps, comm, replicated=False):
    cr = 3.385137501286538e-10
    p, _ = PR.cube_params(n=n)
    lo, hi = shard_range(n, rank, world)
    eng = NumpyShardEngine(n, lo, hi, cr)
    sim = ShardedSimulation(p, rank, world, engine=eng, comm=comm, replicated_detect=replicated)
    sim.upload(*make_state(n))
    tot = None
    for s in range(steps):
        st = sim.timestep(2e-13)
        tot = st if tot is None else {k: tot[k] + st[k] for k in st}
    return sim, tot


def _worker(rank, world, port, n, steps, q, replicated=False):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sim, tot = run_sim(n, rank, world, steps, TorchComm(rank, world), replicated)
        full = sim.download()
        if rank == 0:
            q.put(({k: v for k, v in full.items()}, tot))
    finally:
        dist.destroy_process_group()


def _first_result(q, procs, timeout):
    """Rank 0's result, or a failure as soon as a rank has died; no child outlives the call."""
    import queue
    import time
    try:
        t0 = time.time()
        while True:
            try:
                out = q.get(timeout=1.0)
                break
            except queue.Empty:
                dead = [p for p in procs if p.exitcode not in (None, 0)]
                if dead:
                    pytest.fail(f"a rank exited with code {dead[0].exitcode}")
                if time.time() - t0 > timeout:
                    pytest.fail(f"no result after {timeout} s")
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        return out
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class _NoComm:
    world = 1
    backend = "none"
    shortcut = True

    def allreduce_sum_ints(self, v): return list(v)


# equal and unequal shards; 8 = the rank count of BASELINE configs[4]; detection sharded by index (two collectives per step:
# positions, then the candidate pairs every rank found for its own particles) and, once, the replicated form
@pytest.mark.parametrize("n,world,replicated", [(240, 2, False), (251, 2, False), (251, 3, False), (253, 8, False), (251, 3, True)])
def test_ranks_equal_one_rank(n, world, replicated):
    steps = 6
    ref_sim, ref_tot = run_sim(n, 0, 1, steps, _NoComm())
    ref = ref_sim.engine.download()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, steps, q, replicated)) for r in range(world)]
    for p in procs:
        p.start()
    got, tot = _first_result(q, procs, 120)
    assert ref_tot["n_candidates"] > 0
    for k in KEYS:
        a, b = got[k], ref[k]
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), k          # bitwise, incl. -0.0
    assert np.array_equal(got["flag"], ref["flag"]) and ref["flag"].any()
    for k in ("n_pp", "n_wall"):
        assert tot[k] == ref_tot[k], k


def test_shard_ranges_cover_everything():
    for n in (1, 7, 100, 1000003):
        for w in (1, 2, 3, 8):
            r = [shard_range(n, k, w) for k in range(w)]
            assert r[0][0] == 0 and r[-1][1] == n
            assert all(r[k][1] == r[k + 1][0] for k in range(w - 1))


# ---- energised walls over shards: global hit order and RNG consumption ---------------------------------------------------------
class _Energies:
    cold, hot = 1.0e-21, 2.0e-21

    def gap(self, z):
        return 1.5e-21 + z


def run_temp(n, rank, world, steps, comm):
    import random
    from argon_monte_carlo_amd.dist import ShardedTemperatureSimulation
    from argon_monte_carlo_amd.energised import DirectionSampler
    p, _ = PR.cube_params(n=n)
    lo, hi = shard_range(n, rank, world)
    sim = ShardedTemperatureSimulation(p, rank, world, engine=NumpyShardEngine(n, lo, hi, 3.385137501286538e-10), comm=comm)
    sim.upload(*make_state(n, seed=9))
    sampler = DirectionSampler(np.random.RandomState(3), random.Random(3))
    out = []
    for s in range(steps):
        st, mom, cold, hot, hm, hc, hh = sim.temp_timestep(2e-13, sampler, _Energies())
        out.append((float(mom), float(cold), float(hot), hm, hc, hh, st["n_pp"]))
    return sim, out


def _temp_worker(rank, world, port, n, steps, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sim, out = run_temp(n, rank, world, steps, TorchComm(rank, world))
        full = sim.download()
        if rank == 0:
            q.put((full, out))
    finally:
        dist.destroy_process_group()


class _NoCommVar(_NoComm):
    def allgather_var(self, rows):
        return [np.ascontiguousarray(rows, dtype=np.float64)]


def test_energised_walls_two_ranks_equal_one_rank():
    n, steps = 251, 5
    ref_sim, ref_out = run_temp(n, 0, 1, steps, _NoCommVar())
    ref = ref_sim.engine.download()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_temp_worker, args=(r, 2, port, n, steps, q)) for r in range(2)]
    for p in procs:
        p.start()
    got, out = _first_result(q, procs, 120)
    assert any(o[3] for o in ref_out)                                          # wall hits happened
    assert out == ref_out                                                       # per-step momentum / energy sums, bitwise
    for k in KEYS:
        assert np.array_equal(got[k].view(np.int64), ref[k].view(np.int64)), k


# ---- an error on one shard is an error on every rank ---------------------------------------------------------------------------
def _fields_body(at, rank, world, n, bad):
    """fields() with a particle out of the sampler's range on one shard, after fields_reset, and of a clean state again."""
    p, _ = PR.cube_params(n=n)
    lo, hi = shard_range(n, rank, world)
    sim = ShardedSimulation(p, rank, world, engine=NumpyShardEngine(n, lo, hi, 3.385137501286538e-10), comm=TorchComm(rank, world))
    state = make_state(n)
    state[3] = state[3].copy()
    state[3][bad] = 2.0 ** 14
    sim.upload(*state)
    sim.enable_fields()
    sim.fields_sample()
    first = _outcome(lambda at: sim.fields())
    sim.fields_reset()
    second = _outcome(lambda at: sim.fields())
    sim.upload(*make_state(n))
    sim.fields_sample()
    third = _outcome(lambda at: sim.fields())
    return [(o if o[0] != "ok" else ("ok", o[1]["n_samples"], o[1]["count"].tolist())) for o in (first, second, third)]


@pytest.mark.parametrize("n,world,bad", [(251, 2, 200), (251, 3, 90)])
def test_field_sample_out_of_range_on_one_shard_raises_on_every_rank(n, world, bad):
    """One rank's fields_read fails (a velocity component at 2^14 m/s in its shard): every rank must raise the same
    ArgonMCError naming the particle from the same fields() call — not the owner raise while the others wait in the
    all-reduce — and a fields() after fields_reset() must then succeed everywhere."""
    assert shard_range(n, 1, world)[0] <= bad < shard_range(n, 1, world)[1]
    outs = _run_ranks_outcomes(world, _fields_body, (n, bad), timeout=150.0)
    assert all(o[0] == "ok" for o in outs), outs
    _assert_same_error([o[1][0] for o in outs], -4, f"particle {bad} ")
    counts = [0] * (8 * 8 * 8)
    assert all(o[1][1] == ("ok", 0, counts) for o in outs), outs
    counts[0] = n
    assert all(o[1][2] == ("ok", 1, counts) for o in outs), outs
