"""The samplers, described once: one record per sampler of the particle state (and of the energised pore's surfaces), which
``engine.Engine``, ``sim.Simulation`` and ``dist.ShardedSimulation`` read instead of repeating each other.  A record says how the
sampler is called (the C / engine prefix), where the engine keeps its grid, what a read returns beside the totals, how large the
totals are, and under which keys a checkpoint holds it.  The irregular names (``field_grid``, ``fields_n_samples`` beside
``vdf_counters``) are part of the API and of the checkpoint format: the records keep them, they do not normalise them.

``Controls`` is what the drivers share: enable / disable / sample / reset of a sampler on ``self.engine``.
"""
from __future__ import annotations

import importlib
from dataclasses import dataclass

import numpy as np

from . import _abi


@dataclass(frozen=True)
class Sampler:
    name: str                   # the public plural: enable_<name>, <name>_sample, <name>(), write_<name>
    prefix: str                 # amc_<prefix>_config ... in C, <prefix>_config ... on the engine, <prefix>_grid ... in a checkpoint
    module_name: str            # the module with make_grid, copy_grid, default_grid, grid_to_array, grid_from_array, derive
    grid_type: type             # the ctypes grid
    grid_attr: str              # where the engine keeps the configured grid (None: off)
    shape: object               # (module, grid) -> the totals' shape
    counters: tuple             # the int64 counters a read returns behind the arrays, in the C order
    counter_keys: tuple         # one checkpoint key per counter (scalars); packed: a single key for all of them (an int64 array)
    packed: bool = True
    arrays: tuple = ()          # int64 arrays a read returns between the totals and the counters: (checkpoint key, (module, grid) -> shape)
    particles: tuple = ()       # checkpoint keys of the per-particle arrays (the engine's <particle_read>() returns them)
    particle_read: str = None
    stacked: bool = False       # ... as rows of ONE key, handed to <prefix>_load as one list
    grouped: bool = False       # read returns, and load takes, the counters as one tuple (else one value each)
    cadence: bool = True        # the grid has every and step_offset
    has_sample: bool = True     # amc_<prefix>_sample exists (else the sampler follows the steps)
    energised_only: bool = False
    guarded: bool = True        # a read without a grid raises here (else the library answers)
    grid_word: str = "grid"     # in "totals do not match the configured ..."

    @property
    def module(self):
        return importlib.import_module("." + self.module_name, __package__)

    @property
    def grid_key(self):
        return self.prefix + "_grid"

    @property
    def totals_key(self):
        return self.prefix + "_totals"

    @property
    def keys(self):
        """every checkpoint key of the sampler, the grid's first"""
        return (self.grid_key, self.totals_key) + tuple(k for k, _ in self.arrays) + self.counter_keys + self.particles

    @property
    def c_functions(self):
        """the sampler's entry points in the library"""
        calls = ["config", "read", "load", "reset"] + ["sample"] * self.has_sample
        return tuple(f"amc_{self.prefix}_{c}" for c in calls) + (("amc_" + self.particle_read,) if self.particle_read else ())

    def totals_shape(self, g):
        return tuple(self.shape(self.module, g))

    # ---- the tuple <prefix>_read returns and the arguments <prefix>_load takes, against (totals, arrays, counters, particles) ----
    def join_read(self, totals, arrays, counters):
        return (totals, *arrays, tuple(counters)) if self.grouped else (totals, *arrays, *counters)

    def split_read(self, result):
        rest = result[1 + len(self.arrays):]
        return result[0], tuple(result[1:1 + len(self.arrays)]), tuple(rest[0] if self.grouped else rest)

    def load_args(self, totals, arrays, counters, particles):
        c = (tuple(int(v) for v in counters),) if self.grouped else tuple(int(v) for v in counters)
        p = (list(particles[0]),) if self.stacked else tuple(particles)
        return (totals, *arrays, *c, *p)

    # ---- a checkpoint's entries -------------------------------------------------------------------------------------------------
    def to_checkpoint(self, grid, totals, arrays, counters, particles):
        out = {self.grid_key: self.module.grid_to_array(grid), self.totals_key: totals}
        out.update((k, a) for (k, _), a in zip(self.arrays, arrays))
        if not self.packed:
            out.update((k, int(v)) for k, v in zip(self.counter_keys, counters))
        else:
            out[self.counter_keys[0]] = np.array(counters, dtype=np.int64)
        out.update(zip(self.particles, (np.stack(particles),) if self.stacked else particles))
        return out

    def from_checkpoint(self, z):
        """(grid, the arguments of <prefix>_load) from the checkpoint z; None: it has none of this sampler"""
        if self.grid_key not in z:
            return None
        if not self.packed:
            counters = [int(z[k]) for k in self.counter_keys]
        else:
            counters = [int(v) for v in z[self.counter_keys[0]]]
        args = self.load_args(z[self.totals_key], [z[k] for k, _ in self.arrays], counters, [z[k] for k in self.particles])
        return self.module.grid_from_array(z[self.grid_key]), args


def _bins(g):
    return int(g.n1) * int(g.n2) * int(g.n3)


FIELDS = Sampler("fields", "fields", "fields", _abi.AmcFieldGrid, "field_grid", lambda m, g: (_bins(g), 7, 2),
                 ("n_samples", "n_outside"), ("fields_n_samples", "fields_n_outside"), packed=False)
CORRELATIONS = Sampler("correlations", "corr", "correlations", _abi.AmcCorrGrid, "corr_grid", lambda m, g: m.totals_shape(g),
                       ("n_origins", "n_samples", "n_outside", "window_pos"), ("corr_counters",),
                       particles=("corr_origin",), particle_read="corr_origin", stacked=True, grouped=True)
FLUXES = Sampler("fluxes", "flux", "fluxes", _abi.AmcFluxGrid, "flux_grid", lambda m, g: m.totals_shape(g),
                 ("n_samples", "n_outside"), ("flux_n_samples", "flux_n_outside"), packed=False)
FREE_PATHS = Sampler("free_paths", "mfp", "free_paths", _abi.AmcMfpGrid, "mfp_grid", lambda m, g: m.totals_shape(g),
                     ("n_records", "n_outside", "n_steps"), ("mfp_counters",),
                     arrays=(("mfp_hist", lambda m, g: m.hist_shape(g)),), grouped=True, cadence=False, has_sample=False)
DISTRIBUTIONS = Sampler("distributions", "vdf", "distributions", _abi.AmcVdfGrid, "vdf_grid", lambda m, g: m.totals_shape(g),
                        ("n_samples", "n_outside"), ("vdf_counters",))
TRANSITS = Sampler("transits", "transit", "transits", _abi.AmcTransitGrid, "transit_grid", lambda m, g: m.totals_shape(g),
                   ("n_samples",), ("transit_counters",),
                   particles=("transit_state", "transit_entry"), particle_read="transit_state", grid_word="zones")
PAIRS = Sampler("pairs", "pair", "pairs", _abi.AmcPairGrid, "pair_grid", lambda m, g: m.totals_shape(g),
                ("n_samples", "n_outside", "n_unfiled"), ("pair_counters",))
# (a read without a grid goes to the library with one bin: it answers AMC_ERR_STATE)
SURFACES = Sampler("surface", "surface", "surface", _abi.AmcSurfaceGrid, "surface_grid",
                   lambda m, g: (_abi.AMC_SURFACE_CASES, (1 if g is None else int(g.nbins)) + 1, 3, 2),
                   ("n_steps",), ("surface_n_steps",), packed=False,
                   arrays=(("surface_n_failed", lambda m, g: (_abi.AMC_SURFACE_CASES,)),), cadence=False, has_sample=False,
                   energised_only=True, guarded=False, grid_word="surface grid")

# the cadence hook's order (AMC_SAMPLERS, csrc/amc_host.h), then the energised pore's own
CADENCE = (FIELDS, CORRELATIONS, FLUXES, FREE_PATHS, DISTRIBUTIONS, TRANSITS, PAIRS)
ALL = CADENCE + (SURFACES,)


class Controls:
    """What ``Simulation`` and ``ShardedSimulation`` share: a sampler of ``self.engine`` switched on and off, sampled, reset."""

    def _cadence_offset(self):
        """the step_offset a newly enabled cadence gets (None: the grid's own)"""
        return None

    def _sampler_enable(self, s, grid, **changes):
        g = s.module.default_grid(self.params) if grid is None else grid
        if s.cadence:
            changes["step_offset"] = self._cadence_offset()
        getattr(self.engine, s.prefix + "_config")(s.module.copy_grid(g, **changes))

    def _sampler_disable(self, s):
        getattr(self.engine, s.prefix + "_config")(None)

    def _sampler_sample(self, s):
        getattr(self.engine, s.prefix + "_sample")()

    def _sampler_reset(self, s):
        getattr(self.engine, s.prefix + "_reset")()
