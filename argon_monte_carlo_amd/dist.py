"""Multi-GPU driver: one process per GPU, particles sharded by contiguous index range.

Per step every rank advances only its shard (drift + walls + bounds), then ONE all-gather over RCCL/xGMI hands the
positions of every shard and the velocities that changed to everybody (~28 B per particle).  Detection is sharded by
index: a rank examines its own particles against everybody and keeps the pairs whose partner has the lower index (every
close pair is found once, by the owner of its higher index); a second, small all-gather hands the pairs of all ranks to
everybody, and every rank then resolves the whole system's candidates as a single GPU would (ordered resolve, commit).
(``replicated_detect=True`` or AMC_MG_REPLICATED=1: the round-2 form, detection of the whole system on every rank, one
collective per step — the default below 1.5 million particles in all, where the second collective costs more than the
detection it saves: measured)  All ranks compute every collision from
identical inputs, so cross-shard pairs and chains need no locking, no ownership logic inside the kernels and no further
exchange: the path accumulators and the flag of a particle only feed its own bookkeeping and are meaningful on its owner
alone, which is also the rank that emits the particle's completed paths.  Nothing in the step waits for the host.

``ShardedSimulation`` only needs an *engine* with the ``mg_*`` methods of ``engine.ShardEngine`` and a communicator;
tests/test_dist_gloo.py drives it with a NumPy engine over gloo on CPU.
"""
from __future__ import annotations

import numpy as np

from . import samplers as S


def shard_range(n, rank, world):
    """Contiguous index range [lo, hi) of ``rank``; equal shards when world divides n."""
    base, rem = divmod(int(n), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class TorchComm:
    """torch.distributed collectives on tensors that alias engine memory.  backend "nccl" (= RCCL on ROCm) works on the
    device tensors directly; "gloo" stages GPU tensors through the host (used for rehearsals on one GPU and on CPU)."""

    def __init__(self, rank, world, group=None):
        import torch.distributed as dist
        import os
        self.dist, self.rank, self.world, self.group = dist, rank, world, group
        self.backend = dist.get_backend(group) if dist.is_initialized() else "none"
        # world == 1 normally skips the collectives; AMC_DIST_NOSHORTCUT=1 issues them anyway (single-GPU rehearsal
        # of the RCCL code path: tensors aliasing library memory, all-gather)
        self.shortcut = not (os.environ.get("AMC_DIST_NOSHORTCUT") == "1" and dist.is_initialized())

    def _stage(self, t):
        return t.is_cuda and self.backend != "nccl"

    def allgather_packed(self, send, recv):
        """recv = concatenation of every rank's `send` (equal sizes), in rank order."""
        if self._stage(send):
            import torch
            h = send.cpu()
            parts = [torch.empty_like(h) for _ in range(self.world)]
            self.dist.all_gather(parts, h, group=self.group)
            recv.copy_(torch.cat(parts))
        else:
            self.dist.all_gather_into_tensor(recv, send, group=self.group)

    def gather_shards(self, mine, ranges):
        """all-gather of (possibly unequal) host shards: padded to the longest one."""
        import torch
        m = max(b - a for a, b in ranges)
        dev = "cuda" if self.backend == "nccl" else "cpu"
        pad = torch.zeros(m, dtype=mine.dtype, device=dev)
        pad[:mine.numel()] = mine
        parts = [torch.empty(m, dtype=mine.dtype, device=dev) for _ in ranges]
        self.dist.all_gather(parts, pad, group=self.group)
        return [p[:b - a].cpu() for (a, b), p in zip(ranges, parts)]

    def allreduce_sum_ints(self, values):
        import torch
        if self.world == 1 and self.shortcut:
            return list(values)
        t = torch.tensor(list(values), dtype=torch.int64)
        if self.backend == "nccl":
            t = t.cuda()
        self.dist.all_reduce(t, group=self.group)
        return [int(v) for v in t.cpu().tolist()]

    def allgather_var(self, rows):
        """all-gather of float64 row blocks of different lengths: list of the blocks of all ranks, in rank order."""
        import torch
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if self.world == 1 and self.shortcut:
            return [rows]
        counts = [0] * self.world
        counts[self.rank] = rows.shape[0]
        counts = self.allreduce_sum_ints(counts)
        width = rows.shape[1]
        if sum(counts) == 0:
            return [rows[:0].copy() for _ in counts]
        ranges = [(0, c * width) for c in counts]
        parts = self.gather_shards(torch.from_numpy(rows.reshape(-1)), ranges)
        return [p.numpy().reshape(-1, width) for p in parts]


class ShardedSimulation(S.Controls):
    SHARDED_DETECT_MIN_N = 1_500_000
    SUM_KEYS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors")

    def __init__(self, params, rank, world, backend="nccl", stream_ptr=None, engine=None, comm=None, replicated_detect=None):
        import os
        self.params, self.rank, self.world = params, int(rank), int(world)
        self.n = int(params.n)
        if replicated_detect is None:
            env = os.environ.get("AMC_MG_REPLICATED")
            # sharded detection saves ~0.7 x 54 ns x N of detect time per rank (eight ranks) and costs a second collective
            # (~30 us over RCCL): worth it from ~1.5 million particles in all
            replicated_detect = (env == "1") if env is not None else (self.n < self.SHARDED_DETECT_MIN_N)
        self.replicated_detect = bool(replicated_detect)
        self.lo, self.hi = shard_range(self.n, rank, world)
        if engine is None:
            from .engine import ShardEngine
            engine = ShardEngine(params, self.lo, self.hi)
            if stream_ptr is None:
                # the collectives (and their host staging under gloo) are torch operations: the library's kernels must
                # run on the same stream, or a table could be read before the kernel that fills it has finished
                import torch
                stream_ptr = torch.cuda.current_stream().cuda_stream
            engine.set_stream(stream_ptr)
        self.engine = engine
        self.comm = comm if comm is not None else TorchComm(rank, world)
        self._comm_events = None

    def upload(self, *arrays, **kw):
        """Every rank uploads the full initial state (only its shard of the non-position arrays is ever used)."""
        self.engine.upload(*arrays, **kw)

    def init_synthetic(self, cfg):
        """Initial conditions generated on the device (``ic.device_ic_config``): a particle's numbers depend on the seed and
        its index only, so every rank builds the identical system."""
        self.engine.init_synthetic(cfg)

    def init_separate(self, cfg, min_dist, first_round=1, max_rounds=64):
        """Overlap removal of the synthetic start (``Engine.init_separate``).  Every rank holds the whole system after
        ``init_synthetic`` and the rule depends on nothing but the state, the seed and the regions: every rank makes the same
        call and holds the same state afterwards, without a collective.  Returns the statistics."""
        return self.engine.init_separate(cfg, min_dist, first_round, max_rounds)

    # ---- one step -------------------------------------------------------------------------------------------------------
    def timestep(self, dt, reduce_stats=True, want_stats=True):
        self.engine.mg_local(dt)
        return self._sweep(reduce_stats, want_stats)

    def _sweep(self, reduce_stats=True, want_stats=True):
        """positions (+ changed velocities) of all shards -> everybody, then the sweep of the whole system on every rank"""
        e = self.engine
        if not (self.world == 1 and self.comm.shortcut):
            send, recv = e.exchange_buffers(self.world)
            e.mg_pack(self.world)
            self._allgather(send, recv)
        if self.replicated_detect or (self.world == 1 and self.comm.shortcut) or not hasattr(e, "mg_detect"):
            e.mg_sweep(self.world, self.rank)
        else:
            csend, crecv = e.candidate_buffers(self.world)
            e.mg_detect(self.world, self.rank)              # the other shards in, then my particles against everybody
            self._allgather(csend, crecv)                   # everybody's candidate pairs to everybody
            e.mg_resolve(self.world)                        # the same candidate graph and ordered resolve on every rank
        st = e.mg_finish(want_stats)
        if st is None:
            return None
        if reduce_stats and (self.world > 1 or not self.comm.shortcut):
            tot = self.comm.allreduce_sum_ints([st[k] for k in self.SUM_KEYS])
            st.update(dict(zip(self.SUM_KEYS, tot)))
        return st

    def _allgather(self, send, recv):
        if self._comm_events is None:
            self.comm.allgather_packed(send, recv)
            return
        import torch                            # measurement: the collective bracketed by events on the launch stream
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.comm.allgather_packed(send, recv)
        b.record()
        self._comm_events.append((a, b))

    def profile_collective(self, enable):
        """Bracket every all-gather with events on the launch stream (bench.py's per-kernel pass, GPU engines only)."""
        self._comm_events = [] if enable else None

    def collective_times(self):
        """(total milliseconds, count) of the bracketed all-gathers since profile_collective(True); synchronises."""
        ev = self._comm_events or []
        if not ev:
            return 0.0, 0
        ev[-1][1].synchronize()
        tot = sum(a.elapsed_time(b) for a, b in ev)
        n = len(ev)
        self._comm_events = []
        return tot, n

    def run(self, dt, nsteps):
        acc = None
        nsteps = int(nsteps)
        for k in range(nsteps):
            # counters are cumulative on the device: only the last step reads them back (deltas since the last read)
            st = self.timestep(dt, reduce_stats=False, want_stats=(k == nsteps - 1))
            if st is not None:
                acc = st
        if acc is not None and self.world > 1:
            tot = self.comm.allreduce_sum_ints([acc[k] for k in self.SUM_KEYS])
            acc.update(dict(zip(self.SUM_KEYS, tot)))
        return acc

    # ---- results ---------------------------------------------------------------------------------------------------------
    def download(self):
        """Full state assembled from the owners (every rank returns the same arrays)."""
        st = self.engine.download()
        if self.world == 1:
            return st
        import torch
        out = {}
        ranges = [shard_range(self.n, r, self.world) for r in range(self.world)]
        for k, v in st.items():
            t = torch.from_numpy(np.ascontiguousarray(v))
            parts = self.comm.gather_shards(t[self.lo:self.hi].contiguous(), ranges)
            out[k] = torch.cat(parts).numpy()
        return out

    # ---- sampled fields (fields.py): every rank samples its own shard, the totals are summed exactly ---------------------
    # (enable / disable / sample / reset are samplers.Controls', as in sim.Simulation; a cadence keeps the grid's own step_offset)
    def enable_fields(self, grid=None, every=0):
        self._sampler_enable(S.FIELDS, grid, every=every)

    def disable_fields(self):
        self._sampler_disable(S.FIELDS)

    def fields_sample(self):
        self._sampler_sample(S.FIELDS)

    def fields_reset(self):
        self._sampler_reset(S.FIELDS)

    def _read_summed(self, read, shapes, n_counters, describe, own_if_all_failed=False):
        """``read()`` of this rank -> (its 128-bit word arrays, its counters to sum, whatever else the caller wants back), the
        first two summed over the ranks (``totals.sum_over_ranks``).  ``shapes``: the arrays' shapes, for the zeros a rank whose
        read failed takes part with; None: the sampler is not configured, the error is raised."""
        from ._lib import ArgonMCError
        from .totals import sum_over_ranks
        err = None
        try:
            arrays, counters, rest = read()
        except ArgonMCError as e:
            if shapes is None:
                raise
            err, rest = e, None
            arrays, counters = [np.zeros(s, dtype=np.int64) for s in shapes], [0] * n_counters
        arrays, counters = sum_over_ranks(self.comm, self.world, self.rank, err, arrays, counters, describe, own_if_all_failed)
        return arrays, counters, rest

    @staticmethod
    def _as_words(counts):
        """64-bit counts as (low, high) words with a zero high half: what ``totals.sum_over_ranks`` sums"""
        return np.stack([counts, np.zeros_like(counts)], axis=-1)

    @staticmethod
    def _describe(read, capacity=None):
        """the error for the first failing rank r: status s > 0 is particle s - 1 (named where ``capacity`` has the text), else the code"""
        from ._abi import AMC_ERR_CAPACITY
        from ._lib import ArgonMCError

        def describe(r, s):
            if s > 0 and capacity:
                return ArgonMCError(AMC_ERR_CAPACITY, capacity.format(p=s - 1, r=r))
            return ArgonMCError(AMC_ERR_CAPACITY if s > 0 else s, f"{read} failed on rank {r}")
        return describe

    def fields(self):
        """Simulation.fields() of the whole system (a collective: every rank calls it).  The ranks' 128-bit totals are summed
        as 32-bit limbs in one int64 all-reduce — exact, never through floats — so the integers equal a single engine's.
        A read that fails on one rank (a particle out of the sampler's range lives on one shard) fails on every rank, from
        this same call: the failing rank still takes part in the all-reduce, whose first ``world`` entries carry each rank's
        status — 0, the bad particle's index + 1, or the (negative) error code of any other failure."""
        return self._moments_summed(S.FIELDS)

    def _moments_summed(self, s):
        """``fields()`` / ``fluxes()``: the engine's read of the sampler ``s`` summed over the ranks and derived by its module"""
        g = getattr(self.engine, s.grid_attr)

        def read():
            tot, ns, no = getattr(self.engine, s.prefix + "_read")()
            return [tot], [no], ns
        (tot,), (no,), ns = self._read_summed(
            read, None if g is None else [s.totals_shape(g)], 1,
            self._describe(s.prefix + "_read", "amc_" + s.prefix + ": particle {p} (rank {r}) has a velocity component outside |c| < 2^14 m/s (or NaN); "
                                               "sampling stopped until " + s.name + "_reset"))
        return s.module.derive(g, tot, ns, no, float(self.params.argon_mass), s.module.boltzmann_constant(self.params))

    # ---- sampled correlations (correlations.py): every rank samples its own index range, the totals are summed exactly ------
    def enable_correlations(self, grid=None, every=0, n_lags=None):
        self._sampler_enable(S.CORRELATIONS, grid, every=every, n_lags=n_lags)

    def disable_correlations(self):
        self._sampler_disable(S.CORRELATIONS)

    def correlations_sample(self):
        self._sampler_sample(S.CORRELATIONS)

    def correlations_reset(self):
        self._sampler_reset(S.CORRELATIONS)

    def correlations(self, dt=None, every=None):
        """Simulation.correlations() of the whole system (a collective: every rank calls it).  The ranks' 128-bit totals and
        the outside counter are summed as 32-bit limbs in one int64 all-reduce, exactly as ``fields()`` does, with every rank's
        status in its first ``world`` entries: a read that fails on one rank fails on every rank, from this same call.
        ``dt``: the time step for the lag times (None: the simulation's own where it has one, else 1.0)."""
        from . import correlations as CO
        g = self.engine.corr_grid

        def read():
            tot, c = self.engine.corr_read()
            return [tot], [c[2]], c
        (tot,), (no,), c = self._read_summed(
            read, None if g is None else [CO.totals_shape(g)], 1,
            self._describe("corr_read", "amc_corr: particle {p} (rank {r}) is outside the quantisers' range; "
                                        "sampling stopped until correlations_reset"))
        counters = (c[0], c[1], no, c[3])
        if every is None:
            every = int(g.every) if int(g.every) > 0 else 1
        if dt is None:
            dt = getattr(self, "dt", 1.0)
        return CO.derive(g, tot, counters, dt, every)

    # ---- sampled fluxes (fluxes.py): every rank samples its own index range, the totals are summed exactly -------------------
    def enable_fluxes(self, grid=None, every=0):
        self._sampler_enable(S.FLUXES, grid, every=every)

    def disable_fluxes(self):
        self._sampler_disable(S.FLUXES)

    def fluxes_sample(self):
        self._sampler_sample(S.FLUXES)

    def fluxes_reset(self):
        self._sampler_reset(S.FLUXES)

    def fluxes(self):
        """Simulation.fluxes() of the whole system (a collective: every rank calls it): the ranks' 128-bit totals and the
        outside counter summed as 32-bit limbs in one int64 all-reduce, exactly as ``fields()`` does — a read that fails on one
        rank fails on every rank, from this same call."""
        return self._moments_summed(S.FLUXES)

    # ---- sampled free paths (free_paths.py): every rank bins the records it emitted — owners in its own range ---------------
    def enable_free_paths(self, grid=None, keep_records=False):
        self._sampler_enable(S.FREE_PATHS, grid, keep_records=keep_records)

    def disable_free_paths(self):
        self._sampler_disable(S.FREE_PATHS)

    def free_paths_reset(self):
        self._sampler_reset(S.FREE_PATHS)

    def free_paths(self, dt=None):
        """Simulation.free_paths() of the whole system (a collective: every rank calls it): the ranks' 128-bit totals, their
        histogram counts (as words with a zero high half) and the two record counters summed in one ``totals.sum_over_ranks``
        call, exactly as ``fields()`` does — a read that fails on one rank fails on every rank, from this same call.  The step
        count is every rank's own: they step together.  ``dt``: the time step for the rates; None takes the simulation's own
        where it has one (the energised driver) and raises ValueError where it has none: a rate needs a time."""
        from . import free_paths as FP
        g = self.engine.mfp_grid
        if dt is None:
            dt = getattr(self, "dt", None)
        if dt is None:
            raise ValueError("free_paths(dt=...): this driver has no time step of its own")

        def read():
            tot, hist, (nr, no, ns) = self.engine.mfp_read()
            return [tot, self._as_words(hist)], [nr, no], ns
        (tot, hist), (nr, no), ns = self._read_summed(
            read, None if g is None else [FP.totals_shape(g), FP.hist_shape(g) + (2,)], 2,
            self._describe("mfp_read", "amc_mfp: a free path of particle {p} (rank {r}) is outside [0, 2^-16 m) (or NaN); "
                                       "sampling stopped until free_paths_reset"))
        if ns is None:                  # (unreachable: a failed read has raised above)
            ns = 0
        return FP.derive(g, tot, hist[..., 0], nr, no, ns, dt)

    # ---- sampled velocity distributions (distributions.py): every rank samples its own index range, the counts are summed -----
    def enable_distributions(self, grid=None, every=0):
        self._sampler_enable(S.DISTRIBUTIONS, grid, every=every)

    def disable_distributions(self):
        self._sampler_disable(S.DISTRIBUTIONS)

    def distributions_sample(self):
        self._sampler_sample(S.DISTRIBUTIONS)

    def distributions_reset(self):
        self._sampler_reset(S.DISTRIBUTIONS)

    def distributions(self):
        """Simulation.distributions() of the whole system (a collective: every rank calls it): the ranks' 64-bit counts (as
        words with a zero high half) and the outside counter summed in one ``totals.sum_over_ranks`` call, exactly as
        ``fields()`` does — a read that fails on one rank fails on every rank, from this same call."""
        from . import distributions as VD
        g = self.engine.vdf_grid

        def read():
            tot, ns, no = self.engine.vdf_read()
            return [self._as_words(tot)], [no], ns
        (tot,), (no,), ns = self._read_summed(
            read, None if g is None else [VD.totals_shape(g) + (2,)], 1,
            self._describe("vdf_read", "amc_vdf: particle {p} (rank {r}) has a velocity component outside |c| < 2^14 m/s (or NaN); "
                                       "sampling stopped until distributions_reset"))
        return VD.derive(g, tot[..., 0], ns, no, float(self.params.argon_mass), VD.boltzmann_constant(self.params))

    # ---- sampled transits (transits.py): every rank tracks the particles of its own index range, the totals are summed -------
    def enable_transits(self, grid=None, every=1):
        self._sampler_enable(S.TRANSITS, grid, every=every)

    def disable_transits(self):
        self._sampler_disable(S.TRANSITS)

    def transits_sample(self):
        self._sampler_sample(S.TRANSITS)

    def transits_reset(self):
        self._sampler_reset(S.TRANSITS)

    def transits(self, dt=None, every=None):
        """Simulation.transits() of the whole system (a collective: every rank calls it): the ranks' 128-bit totals summed in
        one ``totals.sum_over_ranks`` call, exactly as ``fields()`` does — a read that fails on one rank fails on every rank,
        from this same call.  Every rank takes the same samples, so the sample counter is any rank's."""
        from . import transits as TR
        g = self.engine.transit_grid
        if dt is None:
            dt = getattr(self, "dt", None)
        if dt is None:
            raise ValueError("transits(dt=...): this driver has no time step of its own")

        def read():
            tot, ns = self.engine.transit_read()
            return [tot], [], ns
        (tot,), _, ns = self._read_summed(
            read, None if g is None else [TR.totals_shape(g)], 0,
            self._describe("transit_read", "amc_transit: particle {p} (rank {r}) has a NaN coordinate; sampling stopped until transits_reset"))
        if ns is None:                  # (unreachable: a failed read has raised above)
            ns = 0
        return TR.derive(g, tot, ns, dt, every)

    # ---- sampled pair distribution (pairs.py): every rank counts the centres of its own index range against ALL particles ------
    def enable_pairs(self, grid=None, every=0):
        self._sampler_enable(S.PAIRS, grid, every=every)

    def disable_pairs(self):
        self._sampler_disable(S.PAIRS)

    def pairs_sample(self):
        self._sampler_sample(S.PAIRS)

    def pairs_reset(self):
        self._sampler_reset(S.PAIRS)

    def pairs(self):
        """Simulation.pairs() of the whole system (a collective: every rank calls it): the ranks' 64-bit counts (as words with
        a zero high half) and the outside counter summed in one ``totals.sum_over_ranks`` call, exactly as ``fields()`` does.
        In the cube every rank holds the final state of every particle when a sample is taken (the sweep is replicated and
        its results are still pending in every rank's slot arrays), so a rank's centres — its own index range — see all their
        neighbours and the sum equals a single context's totals bit for bit.  On a shard of a pore geometry the library refuses
        the sampler (``enable_pairs`` raises AMC_ERR_STATE): there the owner's bounds pass ends the step, and the other shards'
        final state arrives with the next exchange only.
        ``n_unfiled`` counts the particles of the WHOLE system on every rank alike: it is this rank's own value, not a sum."""
        from . import pairs as PA
        g = self.engine.pair_grid

        def read():
            tot, ns, no, nu = self.engine.pair_read()
            return [self._as_words(tot)], [no], (ns, nu)
        (tot,), (no,), (ns, nu) = self._read_summed(read, None if g is None else [PA.totals_shape(g) + (2,)], 1, self._describe("pair_read"))
        return PA.derive(g, tot[..., 0], ns, no, nu, float(self.params.collision_range))

    def histograms(self):
        """Global free-path histograms = sum over ranks (every completed path is emitted by its particle's owner)."""
        counts, tot = self.engine.histograms()
        if self.world == 1:
            return counts, tot
        flat = self.comm.allreduce_sum_ints(list(counts.astype(np.int64).ravel()) + [int(tot)])
        return np.array(flat[:-1], dtype=np.uint64).reshape(counts.shape), flat[-1]


class LocalRanks:
    """All ranks of a sharded job in ONE process on one GPU: the ``ShardEngine`` of every rank (all on one stream), their
    exchange and candidate buffers, and device-to-device copies on that stream in place of the two all-gathers (what the
    collectives deliver, without their time).  Every phase of the step (include/argonmc.h, "multi-GPU") is a method of its
    own, over all ranks; ``step`` is the phases in order.  One rank exchanges nothing: ``mg_local``, ``mg_sweep(1, 0)``,
    ``mg_finish``, the driver's shortcut.  (tools/rehearse_ranks.py; the GPU tests that drive ranks out of order.)"""

    def __init__(self, engines, replicated=True):
        self.engines, self.world, self.replicated = list(engines), len(engines), bool(replicated)
        self.buffers()

    def buffers(self):
        """(again after a call that made an engine reallocate its views)"""
        one = self.world == 1
        self.xb = None if one else [e.exchange_buffers(self.world) for e in self.engines]
        self.cb = None if one or self.replicated else [e.candidate_buffers(self.world) for e in self.engines]
        self.hb = [e.hits_buffers(self.world) for e in self.engines] if all(hasattr(e, "hits_buffers") for e in self.engines) else None

    @staticmethod
    def gather(bufs):
        """every rank's send block into every rank's receive buffer, in rank order"""
        blk = bufs[0][0].numel()
        for _, recv in bufs:
            for q, (send, _) in enumerate(bufs):
                recv[q * blk:(q + 1) * blk].copy_(send)

    def local(self, dt):
        for e in self.engines:
            e.mg_local(dt)

    def pack(self):
        if self.world > 1:
            for e in self.engines:
                e.mg_pack(self.world)

    def exchange(self, candidates=False):
        """the step's first all-gather (behind ``pack``), or its second one: the candidate pairs (behind ``detect``)"""
        if self.world > 1:
            self.gather(self.cb if candidates else self.xb)

    def exchange_hits(self):
        """the third all-gather of a device-RNG step (behind ``mg_hits_pack``): every rank's hit results to every rank"""
        self.gather(self.hb)

    def step_device(self, dt, cfg, row, want_stats=False):
        """One sharded device-RNG step (include/argonmc_shard.h) writing row ``row`` of the run every engine has begun
        (``shard_run_begin``): cases on the shards, the hits exchange, the bounds check, then the sweep's phases."""
        for e in self.engines:
            e.temp_begin(dt)
            e.temp_cases_device(cfg)
            e.mg_hits_pack(self.world)
        self.exchange_hits()
        for e in self.engines:
            e.mg_hits_sums(self.world, row)
            e.mg_bounds()
        self.pack()
        self.exchange()
        if self.replicated or self.world == 1:
            self.sweep()
        else:
            self.detect()
            self.exchange(candidates=True)
            self.resolve()
        return self.finish(want_stats)

    def sweep(self):
        for r, e in enumerate(self.engines):
            e.mg_sweep(self.world, r)

    def detect(self):
        for r, e in enumerate(self.engines):
            e.mg_detect(self.world, r)

    def resolve(self):
        for e in self.engines:
            e.mg_resolve(self.world)

    def finish(self, want_stats=False):
        return [e.mg_finish(want_stats) for e in self.engines]

    def step(self, dt, want_stats=False):
        self.local(dt)
        self.pack()
        self.exchange()
        if self.replicated or self.world == 1:
            self.sweep()
        else:
            self.detect()
            self.exchange(candidates=True)
            self.resolve()
        return self.finish(want_stats)


class _GlobalWallHooks:
    """``drive_energised_cases`` hooks over all shards: the hits of a case are concatenated in rank order — ascending
    particle index, the order of the reference's ``np.where(hits)`` loop (Temp:132-152, 311-553) — on every rank, so
    every rank draws the same random directions from identically seeded streams and applies its own slice."""

    def __init__(self, engine, comm, rank):
        self.e, self.comm, self.rank = engine, comm, rank
        if hasattr(engine, "wall_park"):        # (not the NumPy stand-in of tests/test_dist_gloo.py: it applies every case at its turn)
            self.early_gap, self.wall_park, self.wall_finish = True, self._wall_park, self._wall_finish
            self.wall_hits_again = engine.wall_hits_again

    def wall_hits(self, case):
        idx, normals, contact_z, ok = self.e.wall_hits(case)
        mine = np.column_stack([idx.astype(np.float64), normals.reshape(-1, 3), contact_z, ok.astype(np.float64)])
        parts = self.comm.allgather_var(mine.reshape(-1, 6))
        a = sum(len(p) for p in parts[:self.rank])
        self._mine = slice(a, a + len(parts[self.rank]))        # this rank's hits among all
        allr = np.concatenate(parts) if parts else mine
        return allr[:, 0].astype(np.int32), allr[:, 1:4].copy(), allr[:, 4].copy(), allr[:, 5] != 0.0

    def _gathered(self, dpz, dE):
        allr = np.concatenate(self.comm.allgather_var(np.column_stack([dpz, dE]).reshape(-1, 2)))
        return allr[:, 0].copy(), allr[:, 1].copy()

    def wall_apply(self, case, dirs, Es):
        return self._gathered(*self.e.wall_apply(case, np.asarray(dirs)[self._mine], np.asarray(Es)[self._mine]))

    # the gap case parked at its turn and finished after the last case (energised.drive_energised_cases)
    def _wall_park(self, case, dirs):
        self._parked = self._mine
        self.e.wall_park(case, np.asarray(dirs)[self._mine])

    def _wall_finish(self, case, Es):
        return self._gathered(*self.e.wall_finish(case, np.asarray(Es)[self._parked]))


class ShardedTemperatureSimulation(ShardedSimulation):
    """Temperature_Pore_MC.py's step (Temp:662-853) over index-range shards.  ``sampler`` / ``energies`` are the host
    objects of argon_monte_carlo_amd.energised; every rank must construct them with the same seeds."""

    def __init__(self, params, rank, world, backend="nccl", stream_ptr=None, engine=None, comm=None, device_rng_seed=None,
                 consts=None):
        """``device_rng_seed``: the opt-in, NON-PARITY device-RNG mode (``sim.TemperatureSimulation``) over shards — the draws
        are keyed by (particle, step, case, attempt), so nothing of a step goes through the host: ``temp_timestep_device`` and
        ``run`` replace ``temp_timestep``, and the sampled surfaces work over shards.  ``consts``: the constants the
        parameters were made from (default: ``params.pore_params`` for this particle count).  Every rank passes the same seed."""
        self._device_rng = None
        if device_rng_seed is not None:
            from . import params as PR
            from .energised import device_rng_config
            if consts is None:
                consts = PR.pore_params(n=int(params.n), energised=True)[1]
            self._device_rng = device_rng_config(consts, device_rng_seed)
            self.dt = consts["dt"]
            if engine is None:                      # the device draws read the walls' surface energies from the parameters
                from .energised import SurfaceEnergies
                energies = SurfaceEnergies(consts)
                params.E_cold, params.E_hot = energies.cold, energies.hot
        if engine is None:
            from .engine import ShardEnergisedEngine
            lo, hi = shard_range(int(params.n), rank, world)
            params.reserved0 |= 1                   # the energised masks read prior_*_vals
            engine = ShardEnergisedEngine(params, lo, hi)
            if stream_ptr is None:
                import torch
                stream_ptr = torch.cuda.current_stream().cuda_stream
            engine.set_stream(stream_ptr)
        super().__init__(params, rank, world, backend=backend, stream_ptr=stream_ptr, engine=engine, comm=comm)
        self._hooks = _GlobalWallHooks(self.engine, self.comm, self.rank)

    def temp_timestep(self, dt, sampler, energies, reduce_stats=True):
        from .energised import drive_energised_cases
        e = self.engine
        e.temp_begin(dt)                                                # drift + specular cases on the shard
        res = drive_energised_cases(self._hooks, sampler, energies)     # the seven energised cases, global RNG order
        e.mg_bounds()                                                   # Temp:804
        st = self._sweep(reduce_stats, True)                            # Temp:813-844
        return (st,) + res

    # ---- the device-RNG mode over shards (include/argonmc_shard.h): no host work inside a step ------------------
    def _need_device_rng(self):
        if self._device_rng is None:
            raise ValueError("this ShardedTemperatureSimulation was built without device_rng_seed")

    def set_wall_law(self, kind, alpha_coated=None, alpha_gap=None):
        """``TemperatureSimulation.set_wall_law`` on this rank's context: every rank calls it with the same arguments (host state,
        nothing is communicated)."""
        from .energised import set_wall_law
        set_wall_law(self.engine, self._device_rng, kind, alpha_coated, alpha_gap)

    def _device_step(self, dt, row):
        """cases on the shard | the hit results of all ranks, summed in ascending particle index on every rank | bounds |
        the sweep of the whole system: all enqueued, nothing waits for the host"""
        e, w = self.engine, self.world
        send, recv = e.hits_buffers(w)
        e.temp_begin(dt)                                                # drift + specular cases on the shard
        e.temp_cases_device(self._device_rng)                           # cases 3..9, draws keyed by (particle, step, case, attempt)
        e.mg_hits_pack(w)
        if w == 1 and self.comm.shortcut:
            recv.copy_(send)
        else:
            self._allgather(send, recv)                                 # the third, small collective
        e.mg_hits_sums(w, row)
        e.mg_bounds()                                                   # Temp:804
        self._sweep(False, False)                                       # Temp:813-844, mg_finish without statistics

    def _run_end(self, nsteps):
        """The run's one synchronisation, then ONE all-reduce: every rank's status and counters.  A rank whose run failed still
        takes part, so that every rank raises from this call: its own error when all of them failed (an overflowing hits block
        is seen by every rank's sums kernel: the same message everywhere), else one that names the first failing rank."""
        from ._lib import ArgonMCError
        status, err = [0] * self.world, None
        try:
            st, sums, had = self.engine.shard_run_end(nsteps)
        except ArgonMCError as e:
            err, st = e, dict.fromkeys(self.SUM_KEYS, 0)
            status[self.rank] = min(int(e.code), -1)
        flat = status + [int(st[k]) for k in self.SUM_KEYS]
        if self.world > 1 or not self.comm.shortcut:
            flat = self.comm.allreduce_sum_ints(flat)
        failed = [(r, c) for r, c in enumerate(flat[:self.world]) if c != 0]
        if failed:
            if err is not None and len(failed) == self.world:
                raise err
            r, c = failed[0]
            raise ArgonMCError(c, f"the sharded device-RNG run failed on rank {r}") from err
        st.update(dict(zip(self.SUM_KEYS, flat[self.world:])))
        return st, sums, had

    def run(self, dt, nsteps):
        """Without a seed: ``ShardedSimulation.run``.  With one: ``nsteps`` device-RNG steps enqueued back to back, one
        synchronisation at the end -> (counters summed over steps and ranks, float64[nsteps, 3] per-step sums of the whole
        system, bool[nsteps, 3]) as ``EnergisedEngine.temp_run_device`` returns them, identical on every rank."""
        if self._device_rng is None:
            return super().run(dt, nsteps)
        nsteps = int(nsteps)
        self.engine.shard_run_begin(nsteps)
        for k in range(nsteps):
            self._device_step(dt, k)
        return self._run_end(nsteps)

    def temp_timestep_device(self, dt):
        """One device-RNG step -> the tuple of ``EnergisedEngine.temp_timestep_device`` for the whole system, identical on
        every rank (synchronises, like the single-context call)."""
        self._need_device_rng()
        self.engine.shard_run_begin(1)
        self._device_step(dt, 0)
        st, sums, had = self._run_end(1)
        return (st, float(sums[0, 0]), float(sums[0, 1]), float(sums[0, 2]), bool(had[0, 0]), bool(had[0, 1]), bool(had[0, 2]))

    # ---- sampled surfaces over shards: every rank accumulates its own hits, the totals are summed exactly ----------------------
    def enable_surface(self, grid=None):
        self._need_device_rng()
        self._sampler_enable(S.SURFACES, grid)

    def surface_reset(self):
        self._sampler_reset(S.SURFACES)

    def surface(self):
        """``TemperatureSimulation.surface()`` of the whole system (a collective: every rank calls it).  The ranks' 128-bit
        totals and ``n_failed`` are summed as 32-bit limbs in one int64 all-reduce, whose first ``world`` entries carry each
        rank's status as in ``ShardedSimulation.fields``: a read that fails on one rank fails on every rank, from this call."""
        from . import surface as SU
        g = self.engine.surface_grid

        def read():
            tot, nf, ns = self.engine.surface_read()
            return [tot], [int(v) for v in nf], ns
        (tot,), nf, ns = self._read_summed(read, None if g is None else [(7, int(g.nbins) + 1, 3, 2)], 7, self._describe("surface_read"),
                                           own_if_all_failed=True)
        return SU.derive(tot, ns, self.dt, g, self.params, n_failed=np.array(nf, dtype=np.int64))
