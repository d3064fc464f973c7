"""GPU (-m gpu): a context gives back everything it allocated.  The library records every device allocation of a context
and amc_destroy frees what was recorded; here contexts of every kind, with their lazily built work spaces, are created and
destroyed over and over, and free device memory must end where it started."""
import random

import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime, whose free memory is read below)

from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR

pytestmark = pytest.mark.gpu

WARMUP_ROUNDS = 6           # the runtime's own pools (the hardware queues behind the overlapped run's second stream) grow
ROUNDS = 8                  # over the first few rounds; the reading is taken once they have settled
TOLERANCE = 3 << 20         # bytes: what the runtime itself may still move between two readings


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_contexts_of_every_kind_give_back_their_device_memory(monkeypatch):
    from argon_monte_carlo_amd.energised import DirectionSampler, SurfaceEnergies, device_rng_config
    from argon_monte_carlo_amd.engine import EnergisedEngine, Engine, ShardEngine
    pc, cc = PR.cube_params_for_n(200_000)
    cube = IC.cube_ic(pc, cc, seed=5)
    pp, cp = PR.pore_params(n=200_000)
    pore = IC.pore_ic(pp, cp, seed=6)
    ps, cs = PR.pore_params(n=1_000_000)             # (sharded: candidate blocks of a megabyte and more)
    shard = IC.pore_ic(ps, cs, seed=8)
    monkeypatch.setenv("AMC_MG_CANDIDATES", str(1 << 30))     # (capped at the context's candidate capacity)
    pe, ce = PR.pore_params(n=1_000_000, energised=True)
    pe.reserved0 |= 1
    energised = IC.pore_ic(pe, ce, seed=7)
    energies = SurfaceEnergies(ce)
    pe.E_cold, pe.E_hot = energies.cold, energies.hot
    rng_cfg = device_rng_config(ce, 0x5EED)

    def cube_context():
        e = Engine(pc)
        e.upload(*cube)
        e.timestep(cc["dt"])
        e.close()

    def pore_with_kept_lists():
        monkeypatch.setenv("AMC_LIST_KEEP", "4")
        e = Engine(pp)
        e.upload(*pore)
        e.run(cp["dt"], 3)
        e.close()
        monkeypatch.delenv("AMC_LIST_KEEP")

    def energised_pore():
        e = EnergisedEngine(pe)
        e.upload(*energised)
        e.temp_timestep(ce["dt"], DirectionSampler(np.random.RandomState(7), random.Random(7)), energies)
        e.temp_timestep_device(ce["dt"], rng_cfg)
        e.close()

    def overlapped_pore():
        monkeypatch.setenv("AMC_OVERLAP", "1")
        e = Engine(pp)
        e.upload(*pore)
        e.run(cp["dt"], 3)
        assert e.overlap_stats()["steps"] > 0           # (the run did take the overlapped path)
        e.close()
        monkeypatch.delenv("AMC_OVERLAP")

    def shard_views():
        # (the pore keeps its lists: the exchange view's node pools outgrow the streaming pass's and replace its node records)
        e = ShardEngine(ps, 0, ps.n)
        e.upload(*shard)
        for world in (1, 2):
            e.exchange_buffers(world)
            e.candidate_buffers(world)
        e.close()

    def fields_context():
        e = Engine(pc)
        e.upload(*cube)
        e.fields_config(FL.default_grid(pc))
        e.fields_sample()
        e.close()

    from argon_monte_carlo_amd import correlations as CO, distributions as VD, fluxes as FX, free_paths as FP, pairs as PA, surface as SU, transits as TR
    pa, ca = PR.pore_params(n=50_000, energised=True)         # (all eight samplers: the energised pore has the surfaces too)
    pa.reserved0 |= 1
    pa.E_cold, pa.E_hot = energies.cold, energies.hot
    everything = IC.pore_ic(pa, ca, seed=9)
    rng_all = device_rng_config(ca, 0x5EED)

    def all_samplers():
        e = EnergisedEngine(pa)
        e.upload(*everything)
        e.fields_config(FL.default_grid(pa, every=1))
        e.corr_config(CO.default_grid(pa, every=1))
        e.flux_config(FX.default_grid(pa, every=1))
        e.mfp_config(FP.default_grid(pa))
        e.vdf_config(VD.default_grid(pa, every=1))
        e.transit_config(TR.default_grid(pa, every=1))
        e.pair_config(PA.default_grid(pa, every=3))
        e.surface_config(SU.default_grid(pa))
        e.temp_run_device(ca["dt"], 3, rng_all)
        assert e.pair_read()[1] == 1 and e.surface_read()[2] == 3 and e.mfp_read()[2][2] == 3
        e.close()

    kinds = [cube_context, pore_with_kept_lists, energised_pore, overlapped_pore, shard_views, fields_context, all_samplers]
    for _ in range(WARMUP_ROUNDS):
        for make in kinds:
            make()
    free0 = _free_bytes()
    for _ in range(ROUNDS):
        for make in kinds:
            make()
    lost = free0 - _free_bytes()
    assert lost <= TOLERANCE, f"{lost / 2**20:.1f} MiB of device memory not given back after {ROUNDS} rounds"
