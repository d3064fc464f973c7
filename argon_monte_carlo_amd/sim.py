"""Host-side mirror of the reference's interface for the hot path.

The reference has no functions around its loop body; its "API" is a set of module-global ndarrays
(``x_vals``, ``x_velocities``, ``dist_since_collision`` ... Pore:385-400), four completed-path lists (Pore:408-413),
the per-step counter ``num_collisions_per_step`` (Pore:424) and ONE real function on the p-p path,
``pairwise_particles_in_cell`` (Pore:160-255).  ``Simulation`` exposes exactly those names; ``timestep(dt)`` is one
iteration of ``for i in range(num_timesteps)`` (Pore:416-557 / Cube:175-338) executed by libargonmc.so on the GPU.
"""
from __future__ import annotations

import numpy as np

from . import ic as IC
from . import outputs as OUT
from . import params as PR
from . import samplers as S
from ._lib import ArgonMCError
from .engine import Engine

_NAMES = {"x_vals": "x", "y_vals": "y", "z_vals": "z", "x_velocities": "vx", "y_velocities": "vy",
          "z_velocities": "vz", "dist_since_collision": "d", "dist_x_since_collision": "dx",
          "dist_y_since_collision": "dy", "dist_z_since_collision": "dz", "full_path_traveled": "flag"}


def _write_npz(path, d):
    """A sampler's dict as an .npz (edges as edges_1, edges_2[, edges_3])."""
    e = d.pop("edges")
    np.savez(path, **d, **{f"edges_{k + 1}": v for k, v in enumerate(e)})


class Simulation(S.Controls):
    """``kind``: "cube" (Open_Air_Cube_MC.py), "pore" (Open_Air_Pore_MC.py) — see params.py for the constants."""

    def __init__(self, kind="pore", n=None, sigma=PR.SIGMA, device=0, keep_prior=False, tolerate_fp_errors=False,
                 params=None, consts=None, engine=None):
        """``engine``: drive this context (an ``Engine`` created with the same ``params``) instead of creating one."""
        if params is None:
            if kind == "cube":
                params, consts = PR.cube_params(n=n, sigma=sigma, device=device) if n is None else \
                    PR.cube_params_for_n(n, sigma=sigma, device=device)
            elif kind == "pore":
                params, consts = PR.pore_params(n=n, sigma=sigma, device=device)
            else:
                raise ValueError(kind)
        if keep_prior:
            params.reserved0 |= 1
        if tolerate_fp_errors:
            params.reserved1 |= 1
        self.kind = kind
        self.params, self.consts = params, consts
        self.dt = consts["dt"]
        self.engine = engine if engine is not None else Engine(params)
        self.completed_paths, self.completed_x_paths = [], []
        self.completed_y_paths, self.completed_z_paths = [], []
        self.num_collisions_per_step = 0          # Pore:424 (value of the last step)
        self.total_cols = 0                        # Pore:556
        self.steps_done = 0
        self._cache = None

    # ---- state, under the reference's names ----------------------------------------------------------------------
    def set_state(self, x_vals, y_vals, z_vals, x_velocities, y_velocities, z_velocities, dist_since_collision=None,
                  dist_x_since_collision=None, dist_y_since_collision=None, dist_z_since_collision=None,
                  full_path_traveled=None):
        self.engine.upload(x_vals, y_vals, z_vals, x_velocities, y_velocities, z_velocities, dist_since_collision,
                           dist_x_since_collision, dist_y_since_collision, dist_z_since_collision, full_path_traveled)
        self._cache = None

    def init_synthetic(self, seed=None, device=False, separate=False):
        """Seeded synthetic initial conditions — the reference's own generators are host-side, one-off.
        ``device=True`` generates them on the GPU (counter-based generator: another random stream, no PCIe transfer).
        ``separate=True`` runs ``separate_overlaps`` afterwards, behind either generator."""
        seed = seed if seed is not None else self.consts["seed"]
        self._ic_seed = seed
        if device:
            self.engine.init_synthetic(IC.device_ic_config(self.params, self.consts, seed, "cube" if self.kind == "cube" else "pore"))
            self._cache = None
        else:
            gen = IC.cube_ic if self.kind == "cube" else IC.pore_ic
            self.set_state(*gen(self.params, self.consts, seed))
        if separate:
            self.separate_overlaps()

    def separate_overlaps(self, min_dist=None, max_rounds=64, seed=None):
        """Redraw, on the GPU, every atom that overlaps one of a lower index (``Engine.init_separate``, include/argonmc-ic.h) until
        no pair is closer than ``min_dist`` (default: the collision range).  The new positions come from the device generator
        under ``seed`` (default: the seed of the last ``init_synthetic``) and lie in the atom's own region by its index — the
        host generators store their atoms region by region too.  Raises ``ArgonMCError`` (AMC_ERR_CAPACITY) when pairs are left
        after ``max_rounds`` rounds; the state is then the last round's.  Returns the statistics."""
        if seed is None:
            seed = getattr(self, "_ic_seed", None)
        if seed is None:
            seed = self.consts["seed"]
        cfg = IC.device_ic_config(self.params, self.consts, seed, "cube" if self.kind == "cube" else "pore")
        st = self.engine.init_separate(cfg, self.params.collision_range if min_dist is None else min_dist, 1, max_rounds)
        self._cache = None
        if st["pairs_left"] > 0:
            raise ArgonMCError(-4, "separate_overlaps: %d overlapping pairs (%d atoms to redraw) are left after %d rounds "
                                   "(%d at the start)" % (st["pairs_left"], st["losers_left"], st["rounds"], st["pairs_first"]))
        return st

    def _state(self):
        if self._cache is None:
            self._cache = self.engine.download()
        return self._cache

    def __getattr__(self, name):
        if name in _NAMES:
            v = self._state()[_NAMES[name]]
            return v.astype(bool) if name == "full_path_traveled" else v
        if name in ("prior_x_vals", "prior_y_vals", "prior_z_vals"):
            return self.engine.download_prior()["xyz".index(name[6])]
        raise AttributeError(name)

    # ---- the loop body -----------------------------------------------------------------------------------------------
    def timestep(self, dt=None, collect_paths=True):
        """One iteration of the reference's time loop.  Returns the step's counters."""
        st = self.engine.timestep(self.dt if dt is None else dt)
        self._cache = None
        self.num_collisions_per_step = st["n_pp"] + st["n_wall"]
        self.total_cols += self.num_collisions_per_step
        self.steps_done += 1
        if collect_paths:
            self._collect()
        return st

    def run(self, nsteps, dt=None):
        """``nsteps`` iterations without host synchronisation in between (histograms accumulate on the device)."""
        st = self.engine.run(self.dt if dt is None else dt, nsteps)
        self._cache = None
        self.num_collisions_per_step = None
        self.total_cols += st["n_pp"] + st["n_wall"]
        self.steps_done += nsteps
        return st

    def _collect(self):
        rec = self.engine.drain_paths(sort=True)
        if len(rec):
            self.completed_paths.extend(rec["total"].tolist())
            self.completed_x_paths.extend(rec["px"].tolist())
            self.completed_y_paths.extend(rec["py"].tolist())
            self.completed_z_paths.extend(rec["pz"].tolist())

    # ---- end of run (Pore:559-630) -------------------------------------------------------------------------------------
    def histograms(self):
        """(densities dict, bin edges) from the histograms accumulated on the device."""
        counts, _ = self.engine.histograms()
        if getattr(self, "_hist_base", None) is not None:
            counts = counts + self._hist_base          # paths completed before the checkpoint this run resumed from
        dens = {}
        edges = None
        for row, key in enumerate(["total", "x", "y", "z"]):
            dens[key], edges = OUT.density_from_counts(counts[row], self.params.hist_lo, self.params.hist_hi)
        return dens, edges

    def write_outputs(self, directory="."):
        dens, edges = self.histograms()
        OUT.write_histograms(directory, dens, edges)

    # ---- what the samplers share (samplers.py: one record s per sampler; enable / disable / sample / reset are Controls') -------
    def _cadence_offset(self):
        # (the device's step counter restarts at a resumed checkpoint: the cadence counts from the run's first step)
        return getattr(self, "_step_base", 0)

    def _moments_derive(self, s):
        g = getattr(self.engine, s.grid_attr)
        return s.module.derive(g, *getattr(self.engine, s.prefix + "_read")(), float(self.params.argon_mass), s.module.boltzmann_constant(self.params))

    def _resumed_offset(self, g):
        """The step_offset that continues the cadence of the checkpoint's grid ``g``.  A sample is due when the device's step
        counter plus the offset is a multiple of ``every``: the counter stood at the checkpoint's ``device_step`` when the grid
        was saved and stands at ``steps_done - _step_base`` now (0 after reset_outputs, the checkpoint's step in a device-RNG
        run), so the offset moves by the difference — the grid's own offset is kept, not replaced."""
        if self._saved_device_step is None:         # a checkpoint written before the key: cadences without an offset of their own
            return self._step_base
        return int(g.step_offset) + self._saved_device_step - (self.steps_done - self._step_base)

    def _samplers(self):
        """the records of the samplers this simulation can have"""
        return S.CADENCE

    def _samplers_checkpoint(self):
        """every configured sampler's checkpoint entries (samplers.Sampler.keys): grid, totals, counters, per-particle arrays"""
        out = {}
        for s in self._samplers():
            g = getattr(self.engine, s.grid_attr)
            if g is not None:
                tot, arrays, counters = s.split_read(getattr(self.engine, s.prefix + "_read")())
                particles = getattr(self.engine, s.particle_read)() if s.particle_read else ()
                out.update(s.to_checkpoint(g, tot, arrays, counters, particles))
        return out

    def _samplers_restore(self, z):
        """the inverse, once ``_step_base`` is final (the cadence counts from the run's first step).  A checkpoint without a
        sampler's grid switches that sampler off in the resumed run."""
        for s in self._samplers():
            saved = s.from_checkpoint(z)
            if saved is None:
                self._sampler_disable(s)
                continue
            g, args = saved
            getattr(self.engine, s.prefix + "_config")(s.module.copy_grid(g, step_offset=self._resumed_offset(g)) if s.cadence else g)
            getattr(self.engine, s.prefix + "_load")(*args)

    # ---- sampled fields (fields.py; the reference has no such output) ---------------------------------------
    def enable_fields(self, grid=None, every=0):
        """Sample number density, flow velocity and temperature per bin of ``grid`` (fields.make_grid; None = the geometry's
        default, fields.default_grid) after every ``every``-th step (0: only on ``fields_sample()``).  Starts from zero."""
        self._sampler_enable(S.FIELDS, grid, every=every)

    def disable_fields(self):
        self._sampler_disable(S.FIELDS)

    def fields_sample(self):
        """One sample of the current state now (asynchronous)."""
        self._sampler_sample(S.FIELDS)

    def fields_reset(self):
        self._sampler_reset(S.FIELDS)

    def fields(self):
        """dict: count, number_density (m^-3), velocity and temperature (bins x 3: x, y, z components on a Cartesian grid,
        r, theta, z on an axisymmetric one), T (mean of the three), edges, bin_volume, n_samples, n_outside and the raw
        integer totals (int64[bins, 7, 2], 128-bit (low, high) words).  Bins in linear order (i1 * n2 + i2) * n3 + i3."""
        return self._moments_derive(S.FIELDS)

    def write_fields(self, path):
        """The dict of ``fields()`` as an .npz (edges as edges_1, edges_2[, edges_3])."""
        _write_npz(path, self.fields())

    # ---- sampled correlations (correlations.py; the reference has no such output) ---------------------------
    def enable_correlations(self, grid=None, every=0, n_lags=None):
        """Sample the mean-square displacement and the velocity autocorrelation per group of ``grid`` (correlations.make_grid;
        None = the geometry's default, correlations.default_grid) and lag 0 .. ``n_lags`` (None: the grid's), one sample after
        every ``every``-th step (0: only on ``correlations_sample()``).  Starts from zero; the first sample is a time origin."""
        self._sampler_enable(S.CORRELATIONS, grid, every=every, n_lags=n_lags)

    def disable_correlations(self):
        self._sampler_disable(S.CORRELATIONS)

    def correlations_sample(self):
        """One sample of the current state now (asynchronous): an origin, or the next lag of the window."""
        self._sampler_sample(S.CORRELATIONS)

    def correlations_reset(self):
        self._sampler_reset(S.CORRELATIONS)

    def correlations(self, every=None):
        """dict (correlations.derive): count, msd, vacf and D_msd per (group, lag, component), D_vacf per (group, component),
        lag_time, n_origins, n_samples, n_outside, window_pos and the raw integer totals (int64[groups, n_lags + 1, 7, 2]).
        ``every``: steps between two samples for the lag times (None: the cadence's, or 1 for manual samples)."""
        from . import correlations as CO
        tot, counters = self.engine.corr_read()
        g = self.engine.corr_grid
        if every is None:
            every = int(g.every) if int(g.every) > 0 else 1
        return CO.derive(g, tot, counters, self.dt, every)

    def write_correlations(self, path):
        """The dict of ``correlations()`` as an .npz (edges as edges_1, edges_2[, edges_3])."""
        _write_npz(path, self.correlations())

    # ---- sampled fluxes (fluxes.py; the reference has no such output) -----------------------------------------
    def enable_fluxes(self, grid=None, every=0):
        """Sample the velocity moments behind the pressure tensor, the energy flux and the heat flux per bin of ``grid``
        (fluxes.make_grid; None = the geometry's default, fluxes.default_grid) after every ``every``-th step (0: only on
        ``fluxes_sample()``).  Starts from zero.  Independent of ``enable_fields``."""
        self._sampler_enable(S.FLUXES, grid, every=every)

    def disable_fluxes(self):
        self._sampler_disable(S.FLUXES)

    def fluxes_sample(self):
        """One sample of the current state now (asynchronous)."""
        self._sampler_sample(S.FLUXES)

    def fluxes_reset(self):
        self._sampler_reset(S.FLUXES)

    def fluxes(self):
        """dict (fluxes.derive): count, number_density (m^-3), velocity (bins x 3), pressure_tensor (bins x 3 x 3, Pa), pressure,
        T, energy_flux and heat_flux (bins x 3, W/m^2) — components x, y, z on a Cartesian grid, r, theta, z on an axisymmetric
        one — edges, bin_volume, n_samples, n_outside and the raw integer totals (int64[bins, 2, 7, 2], 128-bit (low, high)
        words).  Bins in linear order (i1 * n2 + i2) * n3 + i3."""
        return self._moments_derive(S.FLUXES)

    def write_fluxes(self, path):
        """The dict of ``fluxes()`` as an .npz (edges as edges_1, edges_2[, edges_3])."""
        _write_npz(path, self.fluxes())

    # ---- sampled free paths (free_paths.py; the reference has four global histograms) -----------------------
    def enable_free_paths(self, grid=None, keep_records=False):
        """Accumulate the completed free paths per bin of ``grid`` (free_paths.make_grid; None = the geometry's default,
        free_paths.default_grid) and ending kind — a wall or another atom — after every step from now on, ``run(k)`` included.
        Starts from zero.  With ``keep_records=False`` the sampler is the path records' reader and empties their buffer after
        every step: the ``completed_*paths`` lists stop growing while the sampler is on (the device histograms are unaffected).
        With ``keep_records=True`` the records stay for ``timestep(collect_paths=True)``; their buffer then has to be drained
        as without the sampler — also before this call if a long ``run`` has filled it: with records missing the first step
        marks the totals lost (``free_paths()`` raises until ``free_paths_reset()``).  Paths completed before the call are not
        binned; a consuming sampler starts by emptying the buffer."""
        self._sampler_enable(S.FREE_PATHS, grid, keep_records=keep_records)

    def disable_free_paths(self):
        self._sampler_disable(S.FREE_PATHS)

    def free_paths_reset(self):
        self._sampler_reset(S.FREE_PATHS)

    def free_paths(self):
        """dict (free_paths.derive): per bin and kind (wall, p-p, both) count, mean_free_path, mean_abs_x/y/z, var_free_path,
        end_rate, hist and hist_density; per bin wall_fraction; hist_edges, edges, bin_volume, n_records, n_outside, n_steps
        and the raw integer totals (int64[bins, 2, 7, 2], 128-bit (low, high) words; int64[bins, 2, hist_bins + 1])."""
        from . import free_paths as FP
        tot, hist, (nr, no, ns) = self.engine.mfp_read()
        return FP.derive(self.engine.mfp_grid, tot, hist, nr, no, ns, self.dt)

    def write_free_paths(self, path):
        """The dict of ``free_paths()`` as an .npz (edges as edges_1, edges_2[, edges_3])."""
        _write_npz(path, self.free_paths())

    # ---- sampled velocity distributions (distributions.py; the reference has no such output) ----------------
    def enable_distributions(self, grid=None, every=0):
        """Sample histograms of the three velocity components and of the speed per region of ``grid``
        (distributions.make_grid; None = the geometry's default, distributions.default_grid) after every ``every``-th step
        (0: only on ``distributions_sample()``).  Starts from zero.  Independent of the other samplers."""
        self._sampler_enable(S.DISTRIBUTIONS, grid, every=every)

    def disable_distributions(self):
        self._sampler_disable(S.DISTRIBUTIONS)

    def distributions_sample(self):
        """One sample of the current state now (asynchronous)."""
        self._sampler_sample(S.DISTRIBUTIONS)

    def distributions_reset(self):
        self._sampler_reset(S.DISTRIBUTIONS)

    def distributions(self):
        """dict (distributions.derive): per region count, pdf (regions x 3 x hist_bins, per m/s — components x, y, z on a
        Cartesian grid, r, theta, z on an axisymmetric one), pdf_speed (regions x hist_bins), the tail counts under, over and
        over_speed, edges_v, edges_speed, the midpoint estimates mean, variance, T_est and mean_speed, n_samples, n_outside,
        the raw counts (int64[regions, 4 * hist_bins + 8]), the spatial edges, kind and shape.  Regions in linear order
        (i1 * n2 + i2) * n3 + i3."""
        from . import distributions as VD
        g = self.engine.vdf_grid
        return VD.derive(g, *self.engine.vdf_read(), float(self.params.argon_mass), VD.boltzmann_constant(self.params))

    def write_distributions(self, path):
        """The dict of ``distributions()`` as an .npz (the spatial edges as edges_1, edges_2[, edges_3])."""
        _write_npz(path, self.distributions())

    # ---- sampled transits (transits.py; the reference has no such output) -----------------------------------
    def enable_transits(self, grid=None, every=1):
        """Track, per zone of ``grid`` (transits.make_grid; None = the geometry's default, transits.default_grid), which side
        every particle entered from and when, and count entries, exits by (entry side, exit side) and residence times, with
        one sample after every ``every``-th step (0: only on ``transits_sample()``).  Starts from zero with every particle
        unknown.  Independent of the other samplers."""
        self._sampler_enable(S.TRANSITS, grid, every=every)

    def disable_transits(self):
        self._sampler_disable(S.TRANSITS)

    def transits_sample(self):
        """One sample of the current state now (asynchronous)."""
        self._sampler_sample(S.TRANSITS)

    def transits_reset(self):
        self._sampler_reset(S.TRANSITS)

    def transits(self, every=None):
        """dict (transits.derive): per zone transmission and return probabilities with their standard error, residence mean
        and variance per (entry side, exit side) in seconds, entry and exit rates, occupancy, the Little's-law residence, the
        number still inside, the residence histogram with its edges, and the raw integers (int64[n_zones, 263, 2], 128-bit
        (low, high) words).  ``every``: steps per sample where the samples were taken by hand."""
        from . import transits as TR
        tot, ns = self.engine.transit_read()
        return TR.derive(self.engine.transit_grid, tot, ns, self.dt, every)

    def write_transits(self, path):
        """The dict of ``transits()`` as an .npz."""
        np.savez(path, **self.transits())

    # ---- sampled pair distribution (pairs.py; the reference has no such output) ----------------------------
    def enable_pairs(self, grid=None, every=0):
        """Sample, per region of ``grid`` (pairs.make_grid; None = the geometry's default, pairs.default_grid), the histogram of
        the distances from every particle of the region to every other particle closer than r_max, and of those pairs that
        still approach, after every ``every``-th step (0: only on ``pairs_sample()``).  A sample is a pair search — several
        steps' worth of time — so ``every`` is meant to be large.  Starts from zero.  Independent of the other samplers."""
        self._sampler_enable(S.PAIRS, grid, every=every)

    def disable_pairs(self):
        self._sampler_disable(S.PAIRS)

    def pairs_sample(self):
        """One sample of the current state now (asynchronous)."""
        self._sampler_sample(S.PAIRS)

    def pairs_reset(self):
        self._sampler_reset(S.PAIRS)

    def pairs(self):
        """dict (pairs.derive): r_edges, r_mid, per region centres, pairs and approaching (the raw integers), g and g_err
        (regions x hist_bins, no wall correction), coordination, overlap_per_centre, approach_fraction, n_samples, n_outside,
        n_unfiled, the raw counts (int64[regions, 1 + 2 * hist_bins]), the spatial edges, kind and shape.  Regions in linear
        order (i1 * n2 + i2) * n3 + i3."""
        from . import pairs as PA
        return PA.derive(self.engine.pair_grid, *self.engine.pair_read(), float(self.params.collision_range))

    def write_pairs(self, path):
        """The dict of ``pairs()`` as an .npz (the spatial edges as edges_1, edges_2[, edges_3])."""
        _write_npz(path, self.pairs())

    # ---- checkpoint / resume (the reference has none: a 10^4-step run is one process lifetime there) ---------------
    def _checkpoint_extra(self):
        """what a subclass adds to a checkpoint (beside the samplers' entries, ``_samplers_checkpoint``)"""
        return {}

    def _restore_extra(self, z):
        """the inverse; it leaves ``_step_base`` final: the samplers are restored behind it"""

    def save_checkpoint(self, path):
        """Everything a later ``load_checkpoint`` needs to continue bit-identically: the particle arrays, the
        completed-path lists, the device histograms and the counters (+ RNG streams and per-step lists for Temp, + for every
        sampler that is on the keys its record lists: ``samplers.Sampler.keys``)."""
        st = self.engine.download()
        self._collect()
        counts, _ = self.engine.histograms()
        base = getattr(self, "_hist_base", None)
        if base is not None:
            counts = counts + base
        np.savez(path, kind=self.kind, n=int(self.params.n), collision_range=float(self.params.collision_range),
                 hist_counts=counts.astype(np.uint64), completed_paths=np.array(self.completed_paths, dtype=np.float64),
                 completed_x_paths=np.array(self.completed_x_paths, dtype=np.float64),
                 completed_y_paths=np.array(self.completed_y_paths, dtype=np.float64),
                 completed_z_paths=np.array(self.completed_z_paths, dtype=np.float64),
                 total_cols=int(self.total_cols), steps_done=int(self.steps_done),
                 device_step=int(self.steps_done) - int(getattr(self, "_step_base", 0)),      # (what the saved grids' step_offset counts from)
                 **{f"state_{k}": v for k, v in st.items()}, **self._checkpoint_extra(), **self._samplers_checkpoint())

    def load_checkpoint(self, path):
        z = np.load(path if str(path).endswith(".npz") else str(path) + ".npz", allow_pickle=False)
        if str(z["kind"]) != self.kind or int(z["n"]) != int(self.params.n) or \
                float(z["collision_range"]) != float(self.params.collision_range):
            raise ValueError("checkpoint was written by a different configuration")
        self.engine.upload(*[z[f"state_{k}"] for k in ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz")],
                           flag=z["state_flag"])
        self.engine.reset_outputs()
        self._hist_base = z["hist_counts"].astype(np.uint64)
        self.completed_paths = z["completed_paths"].tolist()
        self.completed_x_paths = z["completed_x_paths"].tolist()
        self.completed_y_paths = z["completed_y_paths"].tolist()
        self.completed_z_paths = z["completed_z_paths"].tolist()
        self.total_cols, self.steps_done = int(z["total_cols"]), int(z["steps_done"])
        self._step_base = self.steps_done           # (reset_outputs restarted the device's step counter)
        self._saved_device_step = int(z["device_step"]) if "device_step" in z else None
        self._cache = None
        self._restore_extra(z)
        self._samplers_restore(z)

    def close(self):
        self.engine.close()


class TemperatureSimulation(Simulation):
    """Temperature_Pore_MC.py: energised walls, per-step z-momentum / energy transfer and momentum_energy.csv
    (Temp:634-638, 756-758, 929-933).  The random directions come from ``np.random`` / ``random`` (module-level streams
    by default, as in the reference) in strict particle order; see energised.py."""

    def __init__(self, n=None, sigma=PR.SIGMA, device=0, np_rng=None, py_rng=None, params=None, consts=None,
                 device_rng_seed=None):
        """``device_rng_seed``: opt-in, NON-PARITY mode — re-emission directions and gap energies are drawn on the GPU
        (Philox4x32-10 keyed by the seed, Gauss-Legendre Debye integral) instead of from ``np.random`` / ``random`` /
        ``mpmath``; same physics and recipe, different random numbers, no per-case host hand-over."""
        from .energised import DirectionSampler, SurfaceEnergies
        from .engine import EnergisedEngine
        if params is None:
            params, consts = PR.pore_params(n=n, sigma=sigma, energised=True, device=device)
        params.reserved0 |= 1
        self.kind = "temp"
        self.params, self.consts = params, consts
        self.dt = consts["dt"]
        # (the gap-energy workers are forked here, ahead of amc_create: no child of this process inherits a HIP context)
        self.energies = SurfaceEnergies(consts, start_workers=True)
        params.E_cold, params.E_hot = self.energies.cold, self.energies.hot
        self.engine = EnergisedEngine(params)
        self.sampler = DirectionSampler(np_rng, py_rng)
        self._device_rng = None
        if device_rng_seed is not None:
            from .energised import device_rng_config
            self._device_rng = device_rng_config(consts, device_rng_seed)
        self.completed_paths, self.completed_x_paths = [], []
        self.completed_y_paths, self.completed_z_paths = [], []
        self.num_collisions_per_step = 0
        self.total_cols = 0
        self.total_errs = 0
        self.steps_done = 0
        self._cache = None
        self.momentum_z_change_per_step = []          # Temp:634
        self.energy_transfer_hot_per_step = []        # Temp:637
        self.energy_transfer_cold_per_step = []       # Temp:638
        self._zero_flags = []

    def init_synthetic(self, seed=None, device=False, separate=False):
        seed = seed if seed is not None else self.consts["seed"]
        self._ic_seed = seed
        if device:
            self.engine.init_synthetic(IC.device_ic_config(self.params, self.consts, seed, "pore"))
            self._cache = None
        else:
            self.set_state(*IC.pore_ic(self.params, self.consts, seed))
        if separate:
            self.separate_overlaps()

    def timestep(self, dt=None, collect_paths=True):
        if self._device_rng is not None:
            st, mom, cold, hot, had_m, had_c, had_h = self.engine.temp_timestep_device(self.dt if dt is None else dt,
                                                                                       self._device_rng)
        else:
            st, mom, cold, hot, had_m, had_c, had_h = self.engine.temp_timestep(self.dt if dt is None else dt,
                                                                                self.sampler, self.energies)
        self._cache = None
        self.momentum_z_change_per_step.append(mom)
        self.energy_transfer_cold_per_step.append(cold)
        self.energy_transfer_hot_per_step.append(hot)
        self._zero_flags.append((not had_m, not had_c, not had_h))
        self.num_collisions_per_step = st["n_pp"] + st["n_wall"]
        self.total_cols += self.num_collisions_per_step
        self.total_errs += st["n_fp_errors"]
        self.steps_done += 1
        if collect_paths:
            self._collect()
        return st

    def run(self, nsteps, dt=None):
        """``nsteps`` iterations.  With ``device_rng_seed`` nothing in a step waits for the host: the whole run is enqueued at
        once and the per-step sums come back as a series (``EnergisedEngine.temp_run_device``); otherwise a loop of steps."""
        if self._device_rng is None:
            for _ in range(int(nsteps)):
                self.timestep(dt, collect_paths=False)
            return None
        nsteps = int(nsteps)
        st, sums, had = self.engine.temp_run_device(self.dt if dt is None else dt, nsteps, self._device_rng)
        self._cache = None
        self.momentum_z_change_per_step.extend(sums[:, 0].tolist())
        self.energy_transfer_cold_per_step.extend(sums[:, 1].tolist())
        self.energy_transfer_hot_per_step.extend(sums[:, 2].tolist())
        self._zero_flags.extend((not m, not c, not h) for m, c, h in had.tolist())
        self.num_collisions_per_step = None
        self.total_cols += st["n_pp"] + st["n_wall"]
        self.total_errs += st["n_fp_errors"]
        self.steps_done += nsteps
        return st

    # ---- the wall law of the device-RNG mode ---------------------------------------------------------------
    def set_wall_law(self, kind, alpha_coated=None, alpha_gap=None):
        """What a hit of the energised walls does from the next step on: "reference" (the reference's recipe, the default) or
        "maxwell" — with probability alpha a diffuse re-emission at the local wall temperature (Knudsen's cosine law), else a
        specular reflection; None: back to the default.  ``alpha_coated`` / ``alpha_gap`` default to the parameters'.  Needs
        ``device_rng_seed``."""
        from .energised import set_wall_law
        set_wall_law(self.engine, self._device_rng, kind, alpha_coated, alpha_gap)

    def wall_law(self):
        """(name, alpha_coated, alpha_gap) of the law in force."""
        from .energised import WALL_LAWS
        kind, ac, ag = self.engine.wall_law_get()
        return WALL_LAWS[kind], ac, ag

    # ---- sampled surfaces (surface.py; the reference reports three sums per step) -------------------------
    def _samplers(self):
        return S.ALL

    def enable_surface(self, grid=None):
        """Accumulate hits, z-momentum and energy per wall bin of the seven energised surfaces in every step from now on
        (``grid``: surface.make_grid; None = surface.default_grid, 32 bins per surface).  Starts from zero."""
        self._sampler_enable(S.SURFACES, grid)

    def disable_surface(self):
        self._sampler_disable(S.SURFACES)

    def surface(self):
        """dict (surface.derive): per case and bin count, hit_rate, momentum_rate and energy_rate (gas side, per area), the
        per-case totals, edges, bin_area, n_steps, n_failed and the raw integer totals (int64[7, nbins + 1, 3, 2])."""
        from . import surface as SU
        tot, nf, ns = self.engine.surface_read()
        return SU.derive(tot, ns, self.dt, self.engine.surface_grid, self.params, n_failed=nf)

    def write_surface(self, path):
        """The dict of ``surface()`` as an .npz: the integers, the grid and the derived arrays."""
        np.savez(path, **self.surface())

    def _checkpoint_extra(self):
        np_state = self.sampler.np_rng.get_state()
        py_state = self.sampler.py_rng.getstate()
        from .energised import wall_law_checkpoint
        return dict(**wall_law_checkpoint(self.engine),
                    momentum=np.array([float(v) for v in self.momentum_z_change_per_step]),
                    energy_cold=np.array([float(v) for v in self.energy_transfer_cold_per_step]),
                    energy_hot=np.array([float(v) for v in self.energy_transfer_hot_per_step]),
                    zero_flags=np.array(self._zero_flags, dtype=bool).reshape(-1, 3), total_errs=int(self.total_errs),
                    np_rng_keys=np.asarray(np_state[1], dtype=np.uint32),
                    np_rng_rest=np.array([np_state[2], np_state[3]], dtype=np.int64), np_rng_gauss=float(np_state[4]),
                    py_rng_state=np.array(py_state[1], dtype=np.uint64), py_rng_version=int(py_state[0]))

    def _restore_extra(self, z):
        self.momentum_z_change_per_step = z["momentum"].tolist()
        self.energy_transfer_cold_per_step = z["energy_cold"].tolist()
        self.energy_transfer_hot_per_step = z["energy_hot"].tolist()
        self._zero_flags = [tuple(bool(b) for b in row) for row in z["zero_flags"]]
        self.total_errs = int(z["total_errs"])
        from .energised import wall_law_restore
        wall_law_restore(self.engine, z["wall_law"] if "wall_law" in z else None)
        if self._device_rng is not None:
            # the device draws are keyed by the step index: the resumed run counts on from the checkpoint's (the cadence of the
            # sampled fields then needs no offset of its own)
            self.engine.set_step(self.steps_done)
            self._step_base = 0
        self.sampler.np_rng.set_state(("MT19937", z["np_rng_keys"], int(z["np_rng_rest"][0]), int(z["np_rng_rest"][1]),
                                       float(z["np_rng_gauss"])))
        self.sampler.py_rng.setstate((int(z["py_rng_version"]), tuple(int(v) for v in z["py_rng_state"]), None))

    def write_outputs(self, directory="."):
        import os
        from .energised import format_mpf
        super().write_outputs(directory)
        m = [format_mpf(v, z[0]) for v, z in zip(self.momentum_z_change_per_step, self._zero_flags)]
        c = [format_mpf(v, z[1]) for v, z in zip(self.energy_transfer_cold_per_step, self._zero_flags)]
        h = [format_mpf(v, z[2]) for v, z in zip(self.energy_transfer_hot_per_step, self._zero_flags)]
        OUT.write_momentum_energy_csv(os.path.join(directory, "momentum_energy.csv"), m, c, h)


# ---- the one real function boundary of the reference: pairwise_particles_in_cell (Pore:160-255) ---------------------
num_collisions_per_step = None       # injected by init_globals(counter), exactly like Pore:350-352
_cell_engines = {}


def init_globals(counter):
    global num_collisions_per_step
    num_collisions_per_step = counter


def pairwise_particles_in_cell(completed_paths, completed_x_paths, completed_y_paths, completed_z_paths, in_cell,
                               continue_path, continue_x_path, continue_y_path, continue_z_path, has_collided,
                               x_positions_in_cell, y_positions_in_cell, z_positions_in_cell, x_velocities_in_cell,
                               y_velocities_in_cell, z_velocities_in_cell, sigma=PR.SIGMA, device=0):
    """Same signature, argument meaning, return tuple and side effects as the reference function: the per-cell arrays
    are updated as the sequential i>j loop would, completed free paths are appended to the four lists in loop order,
    and the shared counter gets the number of collisions (Pore:244-251).  The pair loop runs on the GPU."""
    if num_collisions_per_step is None:
        raise NameError("name 'num_collisions_per_step' is not defined")     # what the reference raises (Pore:244)
    n = int(np.sum(in_cell))
    cap = 1
    while cap < max(n, 2):
        cap <<= 1
    key = (cap, float(sigma), device)
    eng = _cell_engines.get(key)
    if eng is None:
        p, _ = PR.cell_params(sigma=sigma, n=cap, device=device)
        eng = _cell_engines[key] = Engine(p)
    arrs = [np.ascontiguousarray(a, dtype=np.float64).copy() for a in
            (continue_path, continue_x_path, continue_y_path, continue_z_path)]
    flag = np.ascontiguousarray(np.asarray(has_collided).astype(np.uint8))
    pos = [np.ascontiguousarray(a, dtype=np.float64).copy() for a in
           (x_positions_in_cell, y_positions_in_cell, z_positions_in_cell, x_velocities_in_cell,
            y_velocities_in_cell, z_velocities_in_cell)]
    paths, ncoll = eng.pairwise_cell(arrs[0], arrs[1], arrs[2], arrs[3], flag, *pos)
    with num_collisions_per_step.get_lock():
        num_collisions_per_step.value += ncoll
    completed_paths.extend(paths[:, 0].tolist())
    completed_x_paths.extend(paths[:, 1].tolist())
    completed_y_paths.extend(paths[:, 2].tolist())
    completed_z_paths.extend(paths[:, 3].tolist())
    return (in_cell, arrs[0], arrs[1], arrs[2], arrs[3], flag.astype(bool), pos[0], pos[1], pos[2], pos[3], pos[4],
            pos[5])
