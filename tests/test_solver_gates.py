"""CPU proof that the scenes of tests/solver_gates.py sit on the solvers' gates and are strong enough: verify() re-derives every
listed tie from the restatement alone, and every mutant of tests/solver_mutants.py -- one gate of a restatement made wrong -- returns
something else than the real restatement on at least one scene of its family, in the fields tests/test_solver_gates_gpu.py compares.
A kernel with that mistake therefore fails the GPU test.  The mutants run at the smallest size of each family (the restatement has no
launch shapes)."""
import collections

import pytest

import solver_gates as SG
import solver_mutants as SM

SMALL = 64   # the mutants' scenes: at most one wave of edges, and the scenes of which a family has one size only


def small(s):
    if s["family"] in ("twoview", "mlpnp"):
        return True
    return s["sc"]["Ne"] <= SMALL or "-round" not in s["name"]


@pytest.mark.parametrize("family", SG.FAMILIES)
def test_every_scene_sits_on_its_gates(family):
    scenes = SG.scenes(family)
    assert len({s["name"] for s in scenes}) == len(scenes)
    hit = set()
    for s in scenes:
        assert s["family"] == family and s["ties"], s["name"]
        SG.verify(s)
        hit |= {gate for _, _, gate in s["ties"]}
    assert hit == SG.GATES[family], (family, hit ^ SG.GATES[family])


def test_launch_shapes_and_positions():
    """the sizes and tied positions the kernels' launch shapes ask for"""
    by = collections.defaultdict(set)
    for s in SG.scenes("poseopt"):
        by[s["sc"]["Ne"]] |= {(rnd > 0, edge) for rnd, edge, _ in s["ties"]}
    assert sorted(by) == [12, 257, 1025]   # the 64-thread launch, RUN 2, RUN 0
    for Ne, got in by.items():
        assert got == {(later, e) for later in (False, True) for e in SG.positions(Ne)}, Ne
    for family in ("inertial", "inertial_prev"):
        by = collections.defaultdict(set)
        for s in SG.scenes(family):
            by[s["sc"]["Ne"]] |= {(rnd, edge) for rnd, edge, gate in s["ties"] if gate in ("chi2_far", "chi2_close") and "-round" in s["name"]}
        for Ne in (40, 257):   # one wave; T.run = 2
            assert by[Ne] == {(rnd, e) for rnd in range(4) for e in SG.positions(Ne)}, (family, Ne)
    lanes = {name: [it % SG.TV_LANES for it in its] for name, its in SG.TV_LAYOUTS}
    its = dict(SG.TV_LAYOUTS)
    assert len(set(lanes["same_lane"])) == 1 and len(set(lanes["four_strides"])) == 1 and len(its["four_strides"]) == 4
    a, b = its["lower_iteration_higher_lane"]
    assert a < b and a % SG.TV_LANES > b % SG.TV_LANES
    a, b = its["lower_iteration_lower_lane"]
    assert a < b and a % SG.TV_LANES < b % SG.TV_LANES
    assert all(s["want"]["n_matches"] == SG.TV_N for s in SG.scenes("twoview") if s["sc"]["planted"])
    assert SG.ML_ITERATIONS > SG.ML_TRIP == 256


@pytest.mark.parametrize("family", SG.FAMILIES)
def test_control_equals_the_restatement(family):
    """the unmutated text through the mutants' loader == the imported restatement"""
    s = [s for s in SG.scenes(family) if small(s)][0]
    mod = SM.control(family, SG.REAL[family].__name__)
    assert SG.same_result(SG.run(family, s["sc"], s["kw"], mod), s["want"])


@pytest.mark.parametrize("family", SG.FAMILIES)
def test_every_mutant_is_killed_or_equivalent(family):
    mutants = [m for m in SM.MUTANTS if family in m["families"]]
    assert mutants and len({m["id"] for m in SM.MUTANTS}) == len(SM.MUTANTS)
    scenes = [s for s in SG.scenes(family) if small(s)]
    seen = set()   # one scene of every gate first: a mutant meets the scene aimed at it early
    lead = [s for s in scenes if not {g for _, _, g in s["ties"]} <= seen and not seen.update(g for _, _, g in s["ties"])]
    scenes = lead + [s for s in scenes if s not in lead]
    survivors, not_equivalent = [], []
    for m in mutants:
        mod = SM.load(m, family)
        killed = None
        for s in scenes:
            if not SG.same_result(SG.run(family, s["sc"], s["kw"], mod), s["want"]):
                killed = s["name"]
                break
        if m["equivalent"]:
            if killed:
                not_equivalent.append("%s (%s -> %s) on %s" % (m["id"], m["anchor"], m["repl"], killed))
        elif not killed:
            survivors.append("%s [%s -> %s] %s" % (m["id"], m["anchor"], m["repl"], m["what"]))
    assert not survivors, "mutants the scenes cannot tell from the restatement:\n" + "\n".join(survivors)
    assert not not_equivalent, "marked equivalent but differing on a scene:\n" + "\n".join(not_equivalent)


def test_equivalents_are_few_and_argued():
    eq = [m for m in SM.MUTANTS if m["equivalent"]]
    assert 4 * len(eq) <= len(SM.MUTANTS), (len(eq), len(SM.MUTANTS))
    assert all(len(m["equivalent"]) > 40 for m in eq) and all(len(m["what"]) > 10 for m in SM.MUTANTS)
    for m in SM.MUTANTS:   # every anchor is found exactly once
        SM.mutate(SM.source(m["module"]), m)
