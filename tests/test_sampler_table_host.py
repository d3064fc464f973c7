"""Host (no GPU, no library): the samplers' registry (argon_monte_carlo_amd/samplers.py) against the public API it serves.  The
signatures below are literals taken from the commit before the registry: the documented methods keep them."""
import inspect
import re
from pathlib import Path

from argon_monte_carlo_amd import _lib
from argon_monte_carlo_amd import samplers as S
from argon_monte_carlo_amd.dist import ShardedSimulation, ShardedTemperatureSimulation
from argon_monte_carlo_amd.engine import EnergisedEngine, Engine
from argon_monte_carlo_amd.sim import Simulation, TemperatureSimulation

CADENCED = ("fields", "correlations", "fluxes", "distributions", "transits", "pairs")       # ... have <name>_sample
NAMES = CADENCED + ("free_paths",)


def _table(enable, readers, disable=NAMES, write=True):
    out = dict(enable)
    out.update({"disable_" + n: "(self)" for n in disable})
    out.update({n + "_sample": "(self)" for n in CADENCED})
    out.update({n + "_reset": "(self)" for n in NAMES})
    out.update(readers)
    if write:
        out.update({"write_" + n: "(self, path)" for n in NAMES})
    return out


ENABLE = {"enable_fields": "(self, grid=None, every=0)", "enable_correlations": "(self, grid=None, every=0, n_lags=None)",
          "enable_fluxes": "(self, grid=None, every=0)", "enable_free_paths": "(self, grid=None, keep_records=False)",
          "enable_distributions": "(self, grid=None, every=0)", "enable_transits": "(self, grid=None, every=1)",
          "enable_pairs": "(self, grid=None, every=0)"}
SIMULATION = _table(ENABLE, {"fields": "(self)", "correlations": "(self, every=None)", "fluxes": "(self)", "free_paths": "(self)",
                             "distributions": "(self)", "transits": "(self, every=None)", "pairs": "(self)"})
TEMPERATURE = dict(SIMULATION, enable_surface="(self, grid=None)", disable_surface="(self)", surface="(self)", write_surface="(self, path)")
# (the commit before had disable_free_paths, disable_transits and disable_pairs only)
NEW_SHARDED_DISABLE = ("disable_fields", "disable_correlations", "disable_fluxes", "disable_distributions")
SHARDED = _table(ENABLE, {"fields": "(self)", "correlations": "(self, dt=None, every=None)", "fluxes": "(self)", "free_paths": "(self, dt=None)",
                          "distributions": "(self)", "transits": "(self, dt=None, every=None)", "pairs": "(self)"},
                 disable=("free_paths", "transits", "pairs"), write=False)
SHARDED_TEMPERATURE = dict(SHARDED, enable_surface="(self, grid=None)", surface="(self)", surface_reset="(self)")

ENGINE = {}
for _p in ("fields", "flux", "vdf"):
    ENGINE.update({_p + "_config": "(self, grid)", _p + "_sample": "(self)", _p + "_read": "(self)", _p + "_reset": "(self)",
                   _p + "_load": "(self, totals, n_samples, n_outside)"})
ENGINE.update({"corr_config": "(self, grid)", "corr_sample": "(self)", "corr_read": "(self)", "corr_reset": "(self)", "corr_origin": "(self)",
               "corr_load": "(self, totals, counters, origin=None)",
               "mfp_config": "(self, grid)", "mfp_read": "(self)", "mfp_reset": "(self)", "mfp_load": "(self, totals, hist, counters)",
               "transit_config": "(self, grid)", "transit_sample": "(self)", "transit_read": "(self)", "transit_reset": "(self)",
               "transit_state": "(self)", "transit_load": "(self, totals, n_samples, state=None, entry=None)",
               "pair_config": "(self, grid)", "pair_sample": "(self)", "pair_read": "(self)", "pair_reset": "(self)",
               "pair_load": "(self, totals, n_samples, n_outside, n_unfiled)"})
ENERGISED_ENGINE = dict(ENGINE, surface_config="(self, grid)", surface_read="(self)", surface_reset="(self)",
                        surface_load="(self, totals, n_failed, n_steps)")

# the checkpoint format: the keys are frozen, irregular names included
KEYS = {"fields": ("fields_grid", "fields_totals", "fields_n_samples", "fields_n_outside"),
        "fluxes": ("flux_grid", "flux_totals", "flux_n_samples", "flux_n_outside"),
        "correlations": ("corr_grid", "corr_totals", "corr_counters", "corr_origin"),
        "free_paths": ("mfp_grid", "mfp_totals", "mfp_hist", "mfp_counters"),
        "distributions": ("vdf_grid", "vdf_totals", "vdf_counters"),
        "transits": ("transit_grid", "transit_totals", "transit_counters", "transit_state", "transit_entry"),
        "pairs": ("pair_grid", "pair_totals", "pair_counters"),
        "surface": ("surface_grid", "surface_totals", "surface_n_failed", "surface_n_steps")}


def test_public_sampler_methods_keep_their_signatures():
    for cls, want in ((Simulation, SIMULATION), (TemperatureSimulation, TEMPERATURE), (ShardedSimulation, SHARDED),
                      (ShardedTemperatureSimulation, SHARDED_TEMPERATURE), (Engine, ENGINE), (EnergisedEngine, ENERGISED_ENGINE)):
        assert len(want) >= 30
        for name, sig in want.items():
            fn = inspect.getattr_static(cls, name, None)
            assert inspect.isfunction(fn), (cls.__name__, name)         # a plain method, written out in a class body
            assert str(inspect.signature(fn)) == sig, (cls.__name__, name, str(inspect.signature(fn)))
    # the documented API keeps its docstrings
    for name in ENABLE:
        assert len(getattr(Simulation, name).__doc__) > 100, name


def test_the_sharded_driver_can_switch_every_sampler_off():
    for cls in (ShardedSimulation, ShardedTemperatureSimulation):
        for name in NEW_SHARDED_DISABLE:
            assert str(inspect.signature(getattr(cls, name))) == "(self)", (cls.__name__, name)


def test_registry_entries_name_what_exists():
    table = _lib.all_signatures()
    assert len(S.ALL) == 8 and len({s.name for s in S.ALL}) == len({s.prefix for s in S.ALL}) == len({s.grid_attr for s in S.ALL}) == 8
    for s in S.ALL:
        for fn in s.c_functions:
            assert fn in table, (s.name, fn)
        # ... and nothing of the sampler's in the library is missing from its record
        assert {k for k in table if k.startswith(f"amc_{s.prefix}_")} == set(s.c_functions), s.name
        assert table[f"amc_{s.prefix}_config"][1][1]._type_ is s.grid_type, s.name
        assert (f"amc_{s.prefix}_sample" in table) == s.has_sample, s.name
        for fn in ("make_grid", "copy_grid", "default_grid", "grid_to_array", "grid_from_array", "derive"):
            assert callable(getattr(s.module, fn)), (s.name, fn)
        # the grid round-trips through its checkpoint form and sizes the totals
        g = s.module.grid_from_array(s.module.grid_to_array(s.module.default_grid(_params(s))))
        assert isinstance(g, s.grid_type) and all(int(k) >= 1 for k in s.totals_shape(g)), s.name
        assert hasattr(g, "every") == hasattr(g, "step_offset") == s.cadence, s.name
        assert s.keys == KEYS[s.name], (s.name, s.keys)
        assert hasattr(EnergisedEngine, s.prefix + "_config") and hasattr(Engine, s.prefix + "_config") != s.energised_only, s.name
        assert s.particle_read is None or hasattr(Engine, s.particle_read), s.name
    assert [s.name for s in S.ALL if s.energised_only] == ["surface"] and not S.SURFACES.has_sample


def _params(s):
    from argon_monte_carlo_amd import params as PR
    return PR.pore_params(n=1000, energised=s.energised_only)[0]


def test_cadence_entries_are_in_the_hooks_order():
    want = ["fields", "correlations", "fluxes", "free_paths", "distributions", "transits", "pairs"]
    assert [s.name for s in S.CADENCE] == want and S.ALL == S.CADENCE + (S.SURFACES,)
    # ... which is the order of the one table in the host code
    src = (Path(_lib.__file__).parent / "csrc" / "amc_host.h").read_text()
    body = src[src.index("static const amc_sampler AMC_SAMPLERS[] = {"):]
    body = body[:body.index("\n};")]
    ws = re.findall(r"c->(\w+)[\).]", body)
    assert ws == ["F", "CR", "FX", "MF", "VD", "TR", "PD"], ws
    assert re.findall(r", (amc_\w+)\},", body) == ["amc_fields_enqueue", "amc_corr_step", "amc_flux_enqueue", "amc_mfp_step", "amc_vdf_enqueue",
                                                    "amc_transit_enqueue", "amc_pair_enqueue"]
