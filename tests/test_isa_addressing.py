"""The address space of the wide cluster kernel's memory accesses, read off its gfx950 assembly (no GPU needed; skipped
where hipcc is absent).  A pointer taken out of the LDS copy of the argument block is FLAT unless the source types it
(amc_device.h "address spaces"): a FLAT access counts in vmcnt and lgkmcnt, so every wait for an LDS read behind it waits
for the memory round trip too.  tools/isa_counts.py compiles amc_clusters.hip once per module; the test counts flat_,
global_ and registers only.

Register figures: what the two product instantiations had before the accesses were typed — the
typed form must not cost registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_counts  # noqa: E402

pytestmark = pytest.mark.skipif(isa_counts.hipcc_path() is None, reason="hipcc not found")

# The residue: cw_init_slot's `atomicAnd(&W.sl_hits[s], 0)` (amc_clusters.hip), inlined six times, none on an isolated
# pair's path (its slots are `fresh`).  Typed like its neighbours it costs the pore instantiation 287 VGPRs against the
# 285 it had; DESIGN.md 7 (round 16) has the figures.
FLAT_RESIDUE = 6
# (VGPRs incl. AGPRs, spilled SGPRs) of the parent commit
REGISTERS = {"k_clusters_wide<1, false>": (276, 104), "k_clusters_wide<2, false>": (285, 16)}


@pytest.fixture(scope="module")
def wide():
    res = isa_counts.counts("amc_clusters.hip")
    by_name = {}
    for v in res.values():
        name = v["demangled"].replace("void ", "").split("(")[0]
        by_name[name] = v
    return by_name


@pytest.mark.parametrize("name", sorted(REGISTERS))
def test_product_instantiations_address_memory_as_global(wide, name):
    k = wide[name]
    print(name, {q: k[q] for q in ("instructions", "flat", "global", "ds", "vgprs", "sgpr_spill", "vgpr_spill", "scratch_bytes")})
    assert k["flat"] == FLAT_RESIDUE, k["flat"]
    assert k["global"] >= 500, k["global"]          # (they are there, as global_ instructions: 7 before)


@pytest.mark.parametrize("name", sorted(REGISTERS))
def test_typed_pointers_cost_no_registers(wide, name):
    k = wide[name]
    vgprs, sgpr_spill = REGISTERS[name]
    assert k["vgprs"] <= vgprs, (k["vgprs"], vgprs)
    assert k["sgpr_spill"] <= sgpr_spill, (k["sgpr_spill"], sgpr_spill)
    assert k["vgpr_spill"] == 0 and k["scratch_bytes"] == 0, k


def test_all_four_instantiations_are_covered(wide):
    names = sorted(n for n in wide if n.startswith("k_clusters_wide<"))
    assert len(names) == 4, names
    for n in names:
        assert wide[n]["flat"] == FLAT_RESIDUE, (n, wide[n]["flat"])
