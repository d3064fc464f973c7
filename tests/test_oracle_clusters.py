"""The oracle against the REFERENCE ITSELF on the crafted clusters (tests/golden/func_clusters.npz, made by
`oracle/gen_golden.py --only clusters` from tests/cluster_states.py): every cluster of the catalogue as one cell through the
reference's own pairwise_particles_in_cell, members in ascending index, under the identity and the reversed permutation.
Bar: `pow` bit for bit; `mul` the same hits.  Without this pin, GPU == oracle on these shapes (tests/test_gpu_cluster_limits.py)
would prove nothing about the reference.

Also (CPU only): the catalogue holds every case it claims with the hand-known counts, keeps the distance rule in both
geometries and stays finite through the oracle for the steps the GPU tests run."""
import os

import numpy as np
import pytest

from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd._abi import AMC_ERR_FP
from oracle import gen_golden as GG
from oracle import oracle as O
from tests import cluster_states as CS

FIELDS = GG.CLUSTER_FIELDS
GPU_STEPS = 9           # a stage-wise step, timestep x 2 and run(3), or run(8): the most any GPU test runs on one upload (+ 1)


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "func_clusters.npz"))


def test_fixture_inputs_are_the_builders(G):
    """the fixture still belongs to tests/cluster_states.py (rerun `gen_golden.py --only clusters` after changing a builder)"""
    for k, v in GG.cluster_inputs().items():
        assert np.array_equal(np.asarray(v), G[k]), k


def _cell(G, c, mode, reserved1=0):
    sl = slice(int(G["cl_off"][c]), int(G["cl_off"][c + 1]))
    p = PR.cell_params(n=sl.stop - sl.start)[0]
    p.reserved1 = reserved1
    return sl, O.pair_cell(p, *[G[f"cl_in_{f}"][sl] for f in FIELDS], mode=mode, with_records=True)


def test_oracle_reproduces_the_reference_on_every_cluster(G):
    ncell = len(G["cl_off"]) - 1
    names = [str(n) for n in G["cl_name"]]
    # every case of the catalogue is in the fixture, under both permutations
    cases = set(CS.WITHIN_CASES) | set(CS.HANDOVER)
    for perm in GG.CLUSTER_PERMS:
        assert cases <= {n.split("/")[1] for n in names if n.startswith(perm + "/")}
    raised = 0
    for c in range(ncell):
        sl, (a, pa, nca, rca, ra) = _cell(G, c, "pow")
        _, (b, pb, ncb, rcb, rb) = _cell(G, c, "mul")
        if G["cl_outcome"][c]:
            # the reference raised (equal velocities, a == 0): the oracle reports a failed solve, and leaves the pair alone
            # when it is told to count and continue
            assert rca == rcb == AMC_ERR_FP and names[c].endswith("/pair"), names[c]
            _, (t, pt, nct, rct, _r) = _cell(G, c, "pow", reserved1=1)
            assert rct == 0 and nct == 0 and all(np.array_equal(t[f].astype(np.float64), G[f"cl_in_{f}"][sl]) for f in FIELDS)
            raised += 1
            continue
        assert rca == rcb == 0, names[c]
        assert nca == ncb == G["cl_ncoll"][c], (names[c], nca, ncb)
        for f in FIELDS:
            assert np.array_equal(a[f].astype(np.float64), G[f"cl_out_{f}"][sl]), (names[c], f)
        ref = G["cl_paths"][int(G["cl_path_off"][c]):int(G["cl_path_off"][c + 1])]
        assert np.array_equal(pa, ref.reshape(-1, 4)), names[c]
        # mul: the same hits in the same order — every particle's flag is set, so every hit leaves the records (i, j, 0)
        # and (i, j, 1) — and outputs within rounding of pow's.  The positions of a cluster are ~1e-7 m with differences
        # of ~1e-10 m decided to ~1e-9 relative: 1e-6 of a collision range absolute covers the ulps of the exact squares
        # through a chain of hits
        assert G["cl_in_flag"][sl].all() and len(ra) == 2 * nca
        for key in ("i", "j", "which"):
            assert np.array_equal(ra[key], rb[key]), (names[c], key)
        cr = PR.cell_params(n=2)[0].collision_range
        for f in ("x", "y", "z"):
            np.testing.assert_allclose(b[f], a[f], rtol=0, atol=1e-6 * cr, err_msg=names[c])
    assert raised == len(GG.CLUSTER_PERMS)          # the equal-velocity pair, once per permutation


def test_the_reference_hit_what_the_cases_claim(G):
    """On the FIXTURE: the bystander above the pair is hit and the one below is not, every pull of the cascades happens,
    the conflicting pairs meet, the 16-chain's end reaches its outsider."""
    names = [str(n) for n in G["cl_name"]]
    want = {"pair_pull1": None, "pair_pull2": 3, "pulls_4": 6, "pulls_5": 6, "pulls_low": 2, "pull_depth_2": 4, "pull_depth_3": 5, "pull_depth_4": 6}
    for perm in GG.CLUSTER_PERMS:
        pull1 = [int(G["cl_ncoll"][c]) for c, n in enumerate(names) if n == f"{perm}/pair_pull1"]
        assert sorted(pull1) == [1, 1, 2], (perm, pull1)            # below, between: only the pair; above: the bystander too
        for case, hits in want.items():
            if hits is not None:
                got = [int(G["cl_ncoll"][c]) for c, n in enumerate(names) if n == f"{perm}/{case}"]
                assert got == [hits], (perm, case, got)
        both = [int(G["cl_ncoll"][c]) for c, n in enumerate(names) if n == f"{perm}/conflict_overlay"]
        assert sorted(both) == [2, 3], (perm, both)                 # index order A D B C: B and C meet; A B D C: never tested again
        grid = [int(G["cl_ncoll"][c]) for c, n in enumerate(names) if n == f"{perm}/conflict_grid"]
        assert min(grid) >= 3, (perm, grid)


@pytest.mark.parametrize("kind", CS.KINDS)
@pytest.mark.parametrize("perm", CS.PERMS)
def test_structure_gives_the_hand_known_counts(kind, perm):
    seen = set()
    for which in CS.WHICH:
        s = CS.catalogue(kind, perm, which)
        assert not s.extra["absent"], (which, s.extra["absent"])
        assert s.n <= 400
        st = CS.structure(s)
        site = s.extra["site"]
        assert len(st["pairs"]) <= 400
        for c in st["components"]:
            assert len(set(site[c["particles"]].tolist())) == 1        # a component never spans two sites
        for case, idx in s.cases.items():
            comps = sorted(set(st["comp"][idx].tolist()) - {-1})
            assert comps, (which, case)
            for q in comps:
                c = st["components"][q]
                assert (len(c["particles"]), c["candidates"]) == CS.KNOWN[case], (which, case)
            seen.add(case)
        # bystanders and outsiders are in no close pair before the sweep
        for case, lst in s.extra["roles"].items():
            for roles in lst:
                for r, i in roles.items():
                    if isinstance(r, str) and r[0] in "CDEFO" and case not in ("conflict_overlay", "conflict_grid"):
                        assert st["comp"][i] == -1, (which, case, r)
    assert set(CS.KNOWN) <= seen, set(CS.KNOWN) - seen
    s = CS.catalogue(kind, perm, "within")
    assert set(CS.WITHIN_CASES) <= set(s.cases)
    w = CS.expected_waves(s)
    assert w == {"pair": 6, "3-cluster": 4, "4+-cluster": 8, "not owner": 72}, w
    assert CS.expected_cont(s) == (3, 7)
    w = CS.expected_waves(CS.catalogue(kind, perm, "chain_17"))
    assert w == {"pair": 1, "3-cluster": 0, "4+-cluster": 0, "not owner": 16}, w


@pytest.mark.parametrize("kind", CS.KINDS)
def test_distance_rule_holds(kind):
    """no distance after the drift inside [cr (1 - 2 delta), crp (1 + 2 delta)] — and none between 0.9 and 1.1 cr at all"""
    s0 = CS.catalogue(kind, "identity", "within")
    delta = CS.probe_band(s0.p)
    assert (2.5e-4 < delta < 3.5e-4) if kind == "cube" else (0.9e-2 < delta < 1.1e-2), delta
    for perm in CS.PERMS:
        for which in CS.WHICH:
            s = CS.catalogue(kind, perm, which)
            assert len(CS.distance_rule(s)) == 0, (perm, which, CS.distance_rule(s))
            D = CS._distances(s) / s.p.collision_range
            band = np.triu((D > 0.9 + 1e-9) & (D < 1.1 - 1e-9), k=1)
            assert not band.any(), (perm, which, D[band])


def _hits(rec):
    pp = rec[rec["j"] >= 0]
    return {(int(min(i, j)), int(max(i, j))) for i, j in zip(pp["i"], pp["j"])}


@pytest.mark.parametrize("kind", CS.KINDS)
@pytest.mark.parametrize("perm", CS.PERMS)
def test_catalogue_states_stay_finite_and_at_their_sites(kind, perm):
    for which in CS.WHICH:
        s = CS.catalogue(kind, perm, which)
        o = O.Oracle(s.p, mode="mul")
        a = s.arrays()
        o.upload(*a[:10], flag=a[10])
        site = s.extra["site"]
        for q in range(GPU_STEPS):
            rc, so = o.timestep(s.dt)
            assert rc == 0 and so["n_wall"] == 0, (which, q, so)
            st = o.state()
            for f in O.STATE_FIELDS:
                assert np.isfinite(st[f]).all(), (which, q, f)
            if q == 0:
                assert so["n_pp"] > 0
            for i, j in _hits(o.drain_paths()):
                assert site[i] == site[j], (which, q, i, j)              # nothing at one site reaches another
