"""Thin object wrapper over the C ABI: one ``Engine`` = one ``amc_ctx`` = the particle state resident in HBM."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import samplers as S
from ._abi import AMC_K_NAMES, AmcParams, AmcPathRecord, AmcStepStats, AmcWallLaw, path_record_dtype

_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_u32p = C.POINTER(C.c_uint32)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _f64(a, n):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n,):
        raise ValueError(f"expected float64[{n}], got {a.shape}")
    return a


class Engine:
    def __init__(self, params: AmcParams):
        self.lib = _lib.load()
        self.params = params
        self.n = int(params.n)
        for s in S.ALL:                 # the configured grids (None: off): field_grid, corr_grid, ... surface_grid
            setattr(self, s.grid_attr, None)
        self._ctx = C.c_void_p()
        rc = self.lib.amc_create(C.byref(self._ctx), C.byref(params))
        if rc != 0:
            msg = self.lib.amc_last_error(None)
            raise _lib.ArgonMCError(rc, msg.decode() if msg else "amc_create failed")

    def _ck(self, rc):
        if rc != 0:
            msg = self.lib.amc_last_error(self._ctx)
            raise _lib.ArgonMCError(rc, msg.decode() if msg else "")

    def close(self):
        if self._ctx:
            self.lib.amc_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state -----------------------------------------------------------------------------------------------
    def upload(self, x=None, y=None, z=None, vx=None, vy=None, vz=None, d=None, dx=None, dy=None, dz=None, flag=None):
        arrs = [_f64(a, self.n) for a in (x, y, z, vx, vy, vz, d, dx, dy, dz)]
        f = None
        if flag is not None:
            f = np.ascontiguousarray(np.asarray(flag).astype(np.uint8))
        self._ck(self.lib.amc_upload(self._ctx, *[_d(a) for a in arrs],
                                     None if f is None else f.ctypes.data_as(C.POINTER(C.c_uint8))))

    def init_synthetic(self, cfg):
        """Synthetic initial conditions generated on the device (``ic.device_ic_config``); replaces ``upload``."""
        self._ck(self.lib.amc_init_synthetic(self._ctx, C.byref(cfg)))

    SEPARATE_STATS = ("searches", "rounds", "redrawn", "pairs_first", "losers_first", "pairs_left", "losers_left", "next_round")

    def init_separate(self, cfg, min_dist, first_round=1, max_rounds=64):
        """Overlap removal of a synthetic start on the device (include/argonmc-ic.h): pairs closer than ``min_dist`` are searched
        in the whole system and the atom of the higher index is redrawn from ``cfg``'s seed and regions, round after round.
        Returns the eight statistics by name; ``pairs_left > 0``: the budget of rounds did not suffice."""
        st = (C.c_int64 * len(self.SEPARATE_STATS))()
        self._ck(self.lib.amc_init_separate(self._ctx, C.byref(cfg), float(min_dist), int(first_round), int(max_rounds), st))
        return dict(zip(self.SEPARATE_STATS, (int(v) for v in st)))

    def download(self):
        n = self.n
        arrs = [np.empty(n) for _ in range(10)]
        f = np.empty(n, dtype=np.uint8)
        self._ck(self.lib.amc_download(self._ctx, *[_d(a) for a in arrs], f.ctypes.data_as(C.POINTER(C.c_uint8))))
        keys = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"]
        out = dict(zip(keys, arrs))
        out["flag"] = f
        return out

    def download_prior(self):
        a = [np.empty(self.n) for _ in range(3)]
        self._ck(self.lib.amc_download_prior(self._ctx, *[_d(v) for v in a]))
        return a

    # -- stepping ----------------------------------------------------------------------------------------------
    def timestep(self, dt):
        st = AmcStepStats()
        self._ck(self.lib.amc_timestep(self._ctx, float(dt), C.byref(st)))
        return st.as_dict()

    def run(self, dt, nsteps):
        st = AmcStepStats()
        self._ck(self.lib.amc_run(self._ctx, float(dt), int(nsteps), C.byref(st)))
        return st.as_dict()

    def stage_drift(self, dt):
        self._ck(self.lib.amc_stage_drift(self._ctx, float(dt)))

    def stage_walls(self):
        st = AmcStepStats()
        self._ck(self.lib.amc_stage_walls(self._ctx, C.byref(st)))
        return st.as_dict()

    def stage_bounds(self):
        n = C.c_int64(0)
        self._ck(self.lib.amc_stage_bounds(self._ctx, C.byref(n)))
        return n.value

    def stage_sweep(self):
        st = AmcStepStats()
        self._ck(self.lib.amc_stage_sweep(self._ctx, C.byref(st)))
        return st.as_dict()

    def pairwise_cell(self, cont, cx, cy, cz, flag, x, y, z, vx, vy, vz):
        """One cell through the device pair kernel; arrays are updated IN PLACE (float64 / uint8, contiguous)."""
        n = len(x)
        cap = max(16, 8 * n)
        paths = np.zeros((4, cap))
        npaths = C.c_size_t(0)
        ncoll = C.c_int64(0)
        self._ck(self.lib.amc_pairwise_cell(self._ctx, n, _d(cont), _d(cx), _d(cy), _d(cz),
                                            flag.ctypes.data_as(C.POINTER(C.c_uint8)), _d(x), _d(y), _d(z), _d(vx),
                                            _d(vy), _d(vz), _d(paths), cap, C.byref(npaths), C.byref(ncoll)))
        return paths[:, :npaths.value].T.copy(), ncoll.value

    # -- outputs -------------------------------------------------------------------------------------------------
    def drain_paths(self, sort=True):
        pend = C.c_size_t(0)
        self._ck(self.lib.amc_paths_pending(self._ctx, C.byref(pend)))
        rec = np.zeros(max(1, pend.value), dtype=path_record_dtype())
        got = C.c_size_t(0)
        self._ck(self.lib.amc_drain_paths(self._ctx, rec.ctypes.data_as(C.POINTER(AmcPathRecord)), len(rec),
                                          C.byref(got)))
        rec = rec[:got.value]
        if sort and len(rec):
            # the reference's append order: step, wall cases in evaluation order, then colour groups / cells,
            # inside a cell i ascending, j ascending, particle j before particle i (Pore:168-199)
            rec = rec[np.lexsort((rec["which"], rec["j"], rec["i"], rec["cell"], rec["phase"], rec["step"]))]
        return rec

    def paths_pending(self):
        """Path records waiting in the device buffer (at most its capacity)."""
        pend = C.c_size_t(0)
        self._ck(self.lib.amc_paths_pending(self._ctx, C.byref(pend)))
        return int(pend.value)

    def histograms(self):
        nb = int(self.params.hist_bins)
        counts = np.zeros((4, nb), dtype=np.uint64)
        tot = C.c_uint64(0)
        self._ck(self.lib.amc_histograms(self._ctx, counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tot)))
        return counts, tot.value

    def reset_outputs(self):
        self._ck(self.lib.amc_reset_outputs(self._ctx))

    # -- the samplers (samplers.py): one implementation over a sampler's record s; the public methods below name it -----------------
    def _range_count(self):
        """particles in the context's index range"""
        return int(getattr(self, "hi", self.n)) - int(getattr(self, "lo", 0))

    def _sampler_config(self, s, grid):
        self._ck(getattr(self.lib, f"amc_{s.prefix}_config")(self._ctx, None if grid is None else C.byref(grid)))
        setattr(self, s.grid_attr, None if grid is None else s.grid_type.from_buffer_copy(grid))

    def _sampler_sample(self, s):
        self._ck(getattr(self.lib, f"amc_{s.prefix}_sample")(self._ctx))

    def _sampler_reset(self, s):
        self._ck(getattr(self.lib, f"amc_{s.prefix}_reset")(self._ctx))

    def _sampler_grid(self, s, what):
        g = getattr(self, s.grid_attr)
        if g is None:
            raise _lib.ArgonMCError(-6, f"{s.prefix}_{what} before {s.prefix}_config")
        return g

    def _sampler_read(self, s):
        g = self._sampler_grid(s, "read") if s.guarded else getattr(self, s.grid_attr)
        tot = np.zeros(s.totals_shape(g), dtype=np.int64)
        arrays = [np.zeros(shape(s.module, g), dtype=np.int64) for _, shape in s.arrays]
        c = [C.c_int64(0) for _ in s.counters]
        self._ck(getattr(self.lib, f"amc_{s.prefix}_read")(self._ctx, *[a.ctypes.data_as(_i64p) for a in [tot] + arrays], *[C.byref(v) for v in c]))
        return s.join_read(tot, arrays, [v.value for v in c])

    def _sampler_load(self, s, totals, arrays, counters, particles=(), unconfigured=None):
        """totals and arrays checked against the configured grid (none — unconfigured None: the same ValueError; else the entry
        point's name in the library's error), then the per-particle arrays: (array or None, dtype, shape, what the message calls it)"""
        g = getattr(self, s.grid_attr) if unconfigured is None else self._sampler_grid(s, unconfigured)
        arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (totals, *arrays)]
        shapes = [] if g is None else [s.totals_shape(g)] + [shape(s.module, g) for _, shape in s.arrays]
        if g is None or any(a.size != int(np.prod(sh)) for a, sh in zip(arrs, shapes)):
            raise ValueError(f"totals do not match the configured {s.grid_word}")
        per = [None if a is None else np.ascontiguousarray(a, dtype=dtype) for a, dtype, _, _ in particles]
        for a, (_, dtype, shape, label) in zip(per, particles):
            if a is not None and a.shape != shape:
                raise ValueError(f"expected {np.dtype(dtype).name}[{', '.join(str(k) for k in shape)}]{label}, got {a.shape}")
        ptrs = [None if a is None else a.ctypes.data_as(_u32p if a.dtype == np.uint32 else _dp) for a in per]
        self._ck(getattr(self.lib, f"amc_{s.prefix}_load")(self._ctx, *[a.ctypes.data_as(_i64p) for a in arrs], *[int(v) for v in counters], *ptrs))

    # -- sampled fields (fields.py) ------------------------------------------------------------------------------------------
    def fields_config(self, grid):
        """Sample on ``grid`` (an ``AmcFieldGrid``, fields.make_grid); None switches sampling off.  Starts from zero totals."""
        self._sampler_config(S.FIELDS, grid)

    def fields_sample(self):
        """One sample of the current state, enqueued on the context's stream."""
        self._sampler_sample(S.FIELDS)

    def fields_read(self):
        """(int64[bins, 7, 2] totals as (low, high) words, samples, particles outside); synchronises."""
        return self._sampler_read(S.FIELDS)

    def fields_load(self, totals, n_samples, n_outside):
        self._sampler_load(S.FIELDS, totals, (), (n_samples, n_outside))

    def fields_reset(self):
        self._sampler_reset(S.FIELDS)

    # -- sampled fluxes (fluxes.py) --------------------------------------------------------------------------------------------
    def flux_config(self, grid):
        """Sample on ``grid`` (an ``AmcFluxGrid``, fluxes.make_grid); None switches sampling off.  Starts from zero totals."""
        self._sampler_config(S.FLUXES, grid)

    def flux_sample(self):
        """One sample of the current state, enqueued on the context's stream."""
        self._sampler_sample(S.FLUXES)

    def flux_read(self):
        """(int64[bins, 2, 7, 2] totals as (low, high) words, samples, particles outside); synchronises."""
        return self._sampler_read(S.FLUXES)

    def flux_load(self, totals, n_samples, n_outside):
        self._sampler_load(S.FLUXES, totals, (), (n_samples, n_outside))

    def flux_reset(self):
        self._sampler_reset(S.FLUXES)

    # -- sampled correlations (correlations.py) ----------------------------------------------------------------------
    def corr_config(self, grid):
        """Sample on ``grid`` (an ``AmcCorrGrid``, correlations.make_grid); None switches sampling off.  Starts from zero
        totals; the first sample is a time origin."""
        self._sampler_config(S.CORRELATIONS, grid)

    def corr_sample(self):
        """One sample of the current state at the window position, enqueued on the context's stream."""
        self._sampler_sample(S.CORRELATIONS)

    def corr_read(self):
        """(int64[groups, n_lags + 1, 7, 2] totals as (low, high) words, (n_origins, n_samples, n_outside, window_pos));
        synchronises."""
        return self._sampler_read(S.CORRELATIONS)

    def corr_origin(self):
        """The six origin arrays (x0, y0, z0, vx0, vy0, vz0) of the context's index range."""
        self._sampler_grid(S.CORRELATIONS, "origin")
        arrs = [np.zeros(self._range_count()) for _ in range(6)]
        self._ck(self.lib.amc_corr_origin(self._ctx, *[_d(a) for a in arrs]))
        return arrs

    def corr_load(self, totals, counters, origin=None):
        """The inverse of ``corr_read`` + ``corr_origin``: totals, (n_origins, n_samples, n_outside, window_pos) and the six
        origin arrays (None only at window position 0)."""
        self._sampler_load(S.CORRELATIONS, totals, (), counters,
                           [(a, np.float64, (self._range_count(),), "") for a in ([None] * 6 if origin is None else origin)])

    def corr_reset(self):
        self._sampler_reset(S.CORRELATIONS)

    # -- sampled free paths (free_paths.py) --------------------------------------------------------------
    def mfp_config(self, grid):
        """Sample on ``grid`` (an ``AmcMfpGrid``, free_paths.make_grid); None switches sampling off.  Starts from zero totals,
        at the path records' current end."""
        self._sampler_config(S.FREE_PATHS, grid)

    def mfp_read(self):
        """(int64[bins, 2, 7, 2] totals as (low, high) words, int64[bins, 2, hist_bins + 1] histogram counts, (records binned,
        owners outside, steps)); synchronises."""
        return self._sampler_read(S.FREE_PATHS)

    def mfp_load(self, totals, hist, counters):
        """The inverse of ``mfp_read``: totals, histogram counts and (records binned, owners outside, steps)."""
        self._sampler_load(S.FREE_PATHS, totals, (hist,), counters, unconfigured="read")

    def mfp_reset(self):
        self._sampler_reset(S.FREE_PATHS)

    # -- sampled velocity distributions (distributions.py) -----------------------------------------------
    def vdf_config(self, grid):
        """Sample on ``grid`` (an ``AmcVdfGrid``, distributions.make_grid); None switches sampling off.  Starts from zero totals."""
        self._sampler_config(S.DISTRIBUTIONS, grid)

    def vdf_sample(self):
        """One sample of the current state, enqueued on the context's stream."""
        self._sampler_sample(S.DISTRIBUTIONS)

    def vdf_read(self):
        """(int64[regions, 4 * hist_bins + 8] counts, samples, particles outside); synchronises."""
        return self._sampler_read(S.DISTRIBUTIONS)

    def vdf_load(self, totals, n_samples, n_outside):
        """The inverse of ``vdf_read``."""
        self._sampler_load(S.DISTRIBUTIONS, totals, (), (n_samples, n_outside))

    def vdf_reset(self):
        self._sampler_reset(S.DISTRIBUTIONS)

    # -- sampled transits (transits.py) --------------------------------------------------------------------
    def transit_config(self, grid):
        """Sample on ``grid`` (an ``AmcTransitGrid``, transits.make_grid); None switches sampling off.  Starts from zero
        totals and every particle unknown."""
        self._sampler_config(S.TRANSITS, grid)

    def transit_sample(self):
        """One sample of the current state, enqueued on the context's stream."""
        self._sampler_sample(S.TRANSITS)

    def transit_read(self):
        """(int64[n_zones, 263, 2] totals as (low, high) words, samples); synchronises."""
        return self._sampler_read(S.TRANSITS)

    def transit_state(self):
        """The per-particle arrays of the context's index range: (uint32[count] state words, uint32[n_zones, count] entry indices)."""
        cnt = self._range_count()
        state = np.zeros(cnt, dtype=np.uint32)
        entry = np.zeros((int(self._sampler_grid(S.TRANSITS, "state").n_zones), cnt), dtype=np.uint32)
        self._ck(self.lib.amc_transit_state(self._ctx, state.ctypes.data_as(_u32p), entry.ctypes.data_as(_u32p)))
        return state, entry

    def transit_load(self, totals, n_samples, state=None, entry=None):
        """The inverse of ``transit_read`` + ``transit_state`` (state None: every particle unknown; entry None: zeros)."""
        zones, cnt = int(self._sampler_grid(S.TRANSITS, "load").n_zones), self._range_count()
        self._sampler_load(S.TRANSITS, totals, (), (n_samples,), [(state, np.uint32, (cnt,), " state words"),
                                                                  (entry, np.uint32, (zones, cnt), " entry indices")], unconfigured="load")

    def transit_reset(self):
        self._sampler_reset(S.TRANSITS)

    # -- sampled pair distribution (pairs.py) --------------------------------------------------------------
    def pair_config(self, grid):
        """Sample on ``grid`` (an ``AmcPairGrid``, pairs.make_grid); None switches sampling off.  Starts from zero totals."""
        self._sampler_config(S.PAIRS, grid)

    def pair_sample(self):
        """One sample of the current state, enqueued on the context's stream."""
        self._sampler_sample(S.PAIRS)

    def pair_read(self):
        """(int64[regions, 1 + 2 * hist_bins] counts, samples, particles of the range outside the grid, particles of the system
        unfiled); synchronises."""
        return self._sampler_read(S.PAIRS)

    def pair_load(self, totals, n_samples, n_outside, n_unfiled):
        """The inverse of ``pair_read``."""
        self._sampler_load(S.PAIRS, totals, (), (n_samples, n_outside, n_unfiled))

    def pair_reset(self):
        self._sampler_reset(S.PAIRS)

    # -- measurement -----------------------------------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        """Run on the given hipStream_t; 0 = HIP's NULL stream (torch's default current stream)."""
        if not stream_ptr:
            self._ck(self.lib.amc_use_null_stream(self._ctx))
        else:
            self._ck(self.lib.amc_set_stream(self._ctx, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._ck(self.lib.amc_synchronize(self._ctx))

    def overlap_stats(self):
        """(steps amc_run has overlapped, particles advanced again after a sweep pulled them in, mode, extra list nodes,
        launches of the ordered workgroup so far, steps amc_run has enqueued without it, stalls answered, those raised by
        the last step of their run)."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self.lib.amc_overlap_stats(self._ctx, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(steps=int(out[0]), refiled=int(out[1]), mode=int(out[2]), extra_nodes=int(out[3]),
                    ordered_launches=int(out[4]), on_demand_steps=int(out[5]),
                    stalls=int(out[6]), stalls_at_last_step=int(out[7]))

    def lists_stats(self):
        """The kept per-cell lists as they stand (amc_lists_stats): K (0: not kept), nodes per wave pool, waves with a pool,
        steps since the last full build (-1: no cycle), the cycle's owner (1 the streaming pass, 2 the exchange kernels), sum
        and maximum of the owner's wave counters, full builds since the context was created.  Reads only."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self.lib.amc_lists_stats(self._ctx, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(keep_K=int(out[0]), wave_cap=int(out[1]), waves=int(out[2]), lists_age=int(out[3]), owner=int(out[4]),
                    count_sum=int(out[5]), count_max=int(out[6]), full_builds=int(out[7]))

    def owned_count(self):
        """The objects the context owns as it stands (amc_owned_count): allocations, streams and events.  Reads only."""
        n = C.c_int64(0)
        self._ck(self.lib.amc_owned_count(self._ctx, C.byref(n)))
        return int(n.value)

    def profile(self, on=True):
        self._ck(self.lib.amc_profile(self._ctx, int(on)))

    def kernel_times(self):
        nk = len(AMC_K_NAMES)
        ms = np.zeros(nk)
        cnt = np.zeros(nk, dtype=np.int64)
        self._ck(self.lib.amc_kernel_times(self._ctx, _d(ms), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return {AMC_K_NAMES[k]: (float(ms[k]), int(cnt[k])) for k in range(nk)}


class ShardEngine(Engine):
    """Engine + the multi-GPU entry points (include/argonmc.h, "multi-GPU"): the object dist.ShardedSimulation drives.
    The buffers of the per-step all-gather are exposed as torch tensors that alias the library's device memory."""

    def __init__(self, params, lo, hi):
        super().__init__(params)
        self.lo, self.hi = int(lo), int(hi)
        self._ck(self.lib.amc_set_shard(self._ctx, self.lo, self.hi))

    @staticmethod
    def _wrap(ptr, count, typestr):
        import torch

        class _Dev:
            pass
        d = _Dev()
        d.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(d, device="cuda")

    def exchange_buffers(self, world):
        """(send, recv) tensors of the all-gather: this rank's block (float64[block]: positions of the shard + the list of
        velocity changes) and the blocks of all ranks (float64[world * block])."""
        if getattr(self, "_xb_world", None) != world:
            send, recv, blk = C.c_void_p(), C.c_void_p(), C.c_int64(0)
            self._ck(self.lib.amc_mg_exchange_view(self._ctx, int(world), C.byref(send), C.byref(recv), C.byref(blk)))
            self._xb = (self._wrap(send.value, blk.value, "<f8"), self._wrap(recv.value, blk.value * world, "<f8"))
            self._xb_world = world
        return self._xb

    def mg_local(self, dt):
        self._ck(self.lib.amc_mg_local(self._ctx, float(dt)))

    def mg_pack(self, world):
        self._ck(self.lib.amc_mg_pack(self._ctx, int(world)))

    def mg_sweep(self, world, rank):
        self._ck(self.lib.amc_mg_sweep(self._ctx, int(world), int(rank)))

    def candidate_buffers(self, world):
        """(send, recv) tensors of the step's SECOND all-gather (detection sharded by index): this rank's candidate pairs
        (int32[block]: count, -, then (i, j) pairs) and the blocks of all ranks."""
        if getattr(self, "_cb_world", None) != world:
            send, recv, blk = C.c_void_p(), C.c_void_p(), C.c_int64(0)
            self._ck(self.lib.amc_mg_candidates_view(self._ctx, int(world), C.byref(send), C.byref(recv), C.byref(blk)))
            self._cb = (self._wrap(send.value, blk.value, "<i4"), self._wrap(recv.value, blk.value * world, "<i4"))
            self._cb_world = world
        return self._cb

    def mg_detect(self, world, rank):
        self._ck(self.lib.amc_mg_detect(self._ctx, int(world), int(rank)))

    def mg_resolve(self, world):
        self._ck(self.lib.amc_mg_resolve(self._ctx, int(world)))

    def mg_finish(self, want_stats=True):
        if not want_stats:
            self._ck(self.lib.amc_mg_finish(self._ctx, None))
            return None
        st = AmcStepStats()
        self._ck(self.lib.amc_mg_finish(self._ctx, C.byref(st)))
        return st.as_dict()


class EnergisedEngine(Engine):
    """Engine + the energised-wall hand-over (Temp:705-758): ``wall_hits`` / ``wall_apply`` are the hooks that
    ``energised.drive_energised_cases`` drives once per case."""
    early_gap = True            # wall_hits(case) may be called ahead of its turn (it changes nothing): the gap case's integrals start early

    def temp_begin(self, dt):
        self._ck(self.lib.amc_temp_begin(self._ctx, float(dt)))

    def wall_hits(self, case):
        cap = max(4096, self.n // 8 + 1024)
        buf = getattr(self, "_wall_hit_buffers", None)
        if buf is None or len(buf[0]) != cap:       # (kept across calls: seven allocations of megabytes per step otherwise)
            buf = self._wall_hit_buffers = (np.empty(cap, dtype=np.int32), np.empty((cap, 3)), np.empty(cap))
        idx, normal, cz = buf
        n = C.c_size_t(0)
        self._ck(self.lib.amc_wall_hits(self._ctx, int(case), idx.ctypes.data_as(C.POINTER(C.c_int32)), _d(normal), _d(cz),
                                        cap, C.byref(n)))
        k = n.value
        nm = normal[:k].copy()
        ok = np.any(nm != 0.0, axis=1)          # a zero normal marks a failed contact solve (Temp:472-474)
        return idx[:k].copy(), nm, cz[:k].copy(), ok

    def _wall_results(self, call, case, dirs, Es):
        """amc_wall_apply / amc_wall_finish (the latter takes no directions) -> (dpz[n], dE[n])"""
        Es = np.ascontiguousarray(Es, dtype=np.float64)
        n = len(Es)
        dpz, dE = np.zeros(max(1, n)), np.zeros(max(1, n))
        self._ck(call(self._ctx, int(case), *dirs, _d(Es), n, _d(dpz), _d(dE)))
        return dpz[:n], dE[:n]

    def wall_apply(self, case, dirs, Es):
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        return self._wall_results(self.lib.amc_wall_apply, case, (_d(dirs),), Es)

    # a case parked while its surface energies are still being integrated (energised.drive_energised_cases)
    def wall_park(self, case, dirs):
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        self._ck(self.lib.amc_wall_park(self._ctx, int(case), _d(dirs), len(dirs)))

    def wall_finish(self, case, Es):
        return self._wall_results(self.lib.amc_wall_finish, case, (), Es)

    def wall_hits_again(self):
        self._ck(self.lib.amc_wall_hits_again(self._ctx))

    def temp_end(self):
        st = AmcStepStats()
        self._ck(self.lib.amc_temp_end(self._ctx, C.byref(st)))
        return st.as_dict()

    # ---- opt-in, non-parity: directions / energies drawn on the device (no host hand-over) ---------------------------
    def temp_cases_device(self, cfg):
        self._ck(self.lib.amc_temp_cases_device(self._ctx, C.byref(cfg)))

    def device_results(self, case):
        cap = max(4096, self.n // 64 + 1024)
        idx = np.empty(cap, dtype=np.int32)
        dpz, dE = np.empty(cap), np.empty(cap)
        ok = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        self._ck(self.lib.amc_temp_device_results(self._ctx, int(case), idx.ctypes.data_as(C.POINTER(C.c_int32)), _d(dpz), _d(dE),
                                                  ok.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
        k = n.value
        return idx[:k].copy(), dpz[:k].copy(), dE[:k].copy(), ok[:k].astype(bool)

    def device_draws(self, case):
        cap = max(4096, self.n // 64 + 1024)
        idx = np.empty(cap, dtype=np.int32)
        normal, dirs = np.empty((cap, 3)), np.empty((cap, 3))
        cz, Es = np.empty(cap), np.empty(cap)
        n = C.c_size_t(0)
        self._ck(self.lib.amc_temp_device_draws(self._ctx, int(case), idx.ctypes.data_as(C.POINTER(C.c_int32)), _d(normal), _d(cz),
                                                _d(dirs), _d(Es), cap, C.byref(n)))
        k = n.value
        return idx[:k].copy(), normal[:k].copy(), cz[:k].copy(), dirs[:k].copy(), Es[:k].copy()

    def temp_timestep_device(self, dt, cfg):
        """temp_timestep with the random draws on the device: same return tuple, no per-case host round trip."""
        self.temp_begin(dt)
        self.temp_cases_device(cfg)
        st = self.temp_end()
        sums = (C.c_double * 3)()
        had = (C.c_int32 * 3)()
        self._ck(self.lib.amc_temp_device_sums(self._ctx, sums, had))
        return (st, sums[0], sums[1], sums[2], bool(had[0]), bool(had[1]), bool(had[2]))

    def temp_run_device(self, dt, nsteps, cfg):
        """``nsteps`` device-RNG steps enqueued back to back, one synchronisation at the end.  Returns (summed counters,
        float64[nsteps, 3] per-step sums: z-momentum, energy to the cold walls, energy to the hot walls — the values
        ``temp_timestep_device`` returns step by step —, bool[nsteps, 3]: a hit contributed)."""
        nsteps = int(nsteps)
        st = AmcStepStats()
        self._ck(self.lib.amc_temp_run_device(self._ctx, float(dt), nsteps, C.byref(cfg), C.byref(st)))
        sums = np.zeros((max(nsteps, 1), 3))
        had = np.zeros((max(nsteps, 1), 3), dtype=np.uint8)
        left = C.c_int64(0)
        self._ck(self.lib.amc_temp_series_read(self._ctx, 0, nsteps, _d(sums), had.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(left)))
        return st.as_dict(), sums[:nsteps], had[:nsteps].astype(bool)

    def device_contacts(self, case):
        """(particle indices, contact points [n, 3]) of the last device-RNG step's hits of ``case``, ascending particle index."""
        cap = max(4096, self.n // 64 + 1024)
        idx = np.empty(cap, dtype=np.int32)
        xyz = np.empty((cap, 3))
        n = C.c_size_t(0)
        self._ck(self.lib.amc_temp_device_contacts(self._ctx, int(case), idx.ctypes.data_as(C.POINTER(C.c_int32)), _d(xyz), cap,
                                                   C.byref(n)))
        return idx[:n.value].copy(), xyz[:n.value].copy()

    def wall_contacts(self, case, n):
        """Contact points [n, 3] of the pending ``wall_hits(case)``, in its order."""
        xyz = np.empty((max(1, int(n)), 3))
        self._ck(self.lib.amc_wall_contacts(self._ctx, int(case), _d(xyz), len(xyz)))
        return xyz[:int(n)].copy()

    # ---- sampled surfaces (surface.py): hits, z-momentum and heat per wall bin -----------------------------
    def surface_config(self, grid):
        """Sample on ``grid`` (an ``AmcSurfaceGrid``, surface.make_grid); None switches sampling off.  Starts from zero."""
        self._sampler_config(S.SURFACES, grid)

    def surface_read(self):
        """(int64[7, nbins + 1, 3, 2] totals as (low, high) words, int64[7] failed contact solves, steps); synchronises."""
        return self._sampler_read(S.SURFACES)

    def surface_load(self, totals, n_failed, n_steps):
        self._sampler_load(S.SURFACES, totals, (n_failed,), (n_steps,))

    def surface_reset(self):
        self._sampler_reset(S.SURFACES)

    def set_step(self, step):
        """Index of the next step: the step word of the device draws (a resumed run continues the interrupted one's)."""
        self._ck(self.lib.amc_set_step(self._ctx, int(step)))

    # ---- the wall law of the device-RNG steps (include/argonmc-walllaw.h) ------------------------------------
    def wall_law(self, kind=None, alpha_coated=None, alpha_gap=None):
        """Set the law the next device-RNG steps apply to a hit: ``kind`` AMC_WALL_LAW_REFERENCE / AMC_WALL_LAW_MAXWELL (None:
        back to the reference law, as never set); the two alpha default to the parameters' ``alpha_coated`` / ``alpha_gap``."""
        if kind is None:
            self._ck(self.lib.amc_temp_wall_law(self._ctx, None))
            return
        law = AmcWallLaw()
        law.struct_size, law.kind = C.sizeof(AmcWallLaw), int(kind)
        law.alpha_coated = float(self.params.alpha_coated if alpha_coated is None else alpha_coated)
        law.alpha_gap = float(self.params.alpha_gap if alpha_gap is None else alpha_gap)
        self._ck(self.lib.amc_temp_wall_law(self._ctx, C.byref(law)))

    def wall_law_get(self):
        """(kind, alpha_coated, alpha_gap) of the law in force."""
        law = AmcWallLaw()
        self._ck(self.lib.amc_temp_wall_law_get(self._ctx, C.byref(law)))
        return int(law.kind), float(law.alpha_coated), float(law.alpha_gap)

    def temp_timestep(self, dt, sampler, energies):
        """One iteration of Temperature_Pore_MC.py's loop (Temp:662-853)."""
        from .energised import drive_energised_cases
        self.temp_begin(dt)
        res = drive_energised_cases(self, sampler, energies)
        st = self.temp_end()
        return (st,) + res


class ShardEnergisedEngine(ShardEngine, EnergisedEngine):
    """Energised walls on a shard: ``temp_begin`` / ``wall_hits`` / ``wall_apply`` act on the owned index range,
    ``mg_bounds`` is the bounds check between the walls and the sweep (Temp:804); the sweep is ShardEngine's."""

    def mg_bounds(self):
        self._ck(self.lib.amc_mg_bounds(self._ctx))

    # ---- the device-RNG mode over shards (include/argonmc_shard.h) -------------------------------------------
    def hits_buffers(self, world):
        """(send, recv) tensors of the step's THIRD all-gather (device-RNG mode): this rank's hit results (int64[block]: seven
        counts, then per case particle | ok << 32, dp_z and dE as 8-byte words) and the blocks of all ranks."""
        if getattr(self, "_hb_world", None) != world:
            send, recv, blk = C.c_void_p(), C.c_void_p(), C.c_int64(0)
            self._ck(self.lib.amc_mg_hits_view(self._ctx, int(world), C.byref(send), C.byref(recv), C.byref(blk)))
            self._hb = (self._wrap(send.value, blk.value, "<i8"), self._wrap(recv.value, blk.value * world, "<i8"))
            self._hb_world = world
        return self._hb

    def mg_hits_pack(self, world):
        self._ck(self.lib.amc_mg_hits_pack(self._ctx, int(world)))

    def mg_hits_sums(self, world, row):
        self._ck(self.lib.amc_mg_hits_sums(self._ctx, int(world), int(row)))

    def shard_run_begin(self, nsteps):
        """Size the per-step series for ``nsteps`` sharded device-RNG steps and clear the overflow words."""
        self._ck(self.lib.amc_temp_shard_run_begin(self._ctx, int(nsteps)))

    def shard_run_end(self, nsteps):
        """The run's one synchronisation -> (this rank's counters summed over the steps, float64[nsteps, 3] sums of the whole
        system, bool[nsteps, 3]: a hit contributed) — the rows ``EnergisedEngine.temp_run_device`` returns."""
        nsteps = int(nsteps)
        st = AmcStepStats()
        self._ck(self.lib.amc_temp_shard_run_end(self._ctx, nsteps, C.byref(st)))
        sums = np.zeros((max(nsteps, 1), 3))
        had = np.zeros((max(nsteps, 1), 3), dtype=np.uint8)
        left = C.c_int64(0)
        self._ck(self.lib.amc_temp_series_read(self._ctx, 0, nsteps, _d(sums), had.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(left)))
        return st.as_dict(), sums[:nsteps], had[:nsteps].astype(bool)
