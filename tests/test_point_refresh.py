"""tests/point_refresh_ref.py, the normative restatement of SPEC DECISION S26: every case of the planted graph gives what its comment in
tests/point_refresh_scenarios.py works out by hand; every mutant of the restatement changes the outputs of the cases planted for it and
of no other case; and on the random graph the restatement's selection equals the reference's own form (fill the matrix, sort every
row).  So the exact comparison of the GPU outputs with the restatement says something about each rule.  No GPU."""
import numpy as np
import pytest

import point_refresh_ref as P
import point_refresh_scenarios as S


def one(rg, p, what=3, mutant=None):
    return P.refresh_point(rg, p, what, mutant)


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k], np.asarray(a[k]).dtype).tobytes() for k in a)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_planted_case_gives_what_was_worked_out_by_hand(name):
    rg = S.planted_graph()
    c = S.CASES[name]
    before = S.state(rg)
    got = one(rg, c["p"])
    want = S.expected(rg, name)
    print(name, got)
    assert same({k: got[k] for k in want}, want), (got, want)
    after = S.state(rg)
    assert [i for i in range(len(before)) if before[i] != after[i]] == ([c["p"]] if want["status"] else [])
    q = rg.point(c["p"])
    if want["status"] & 2:                                               # the descriptor is the chosen observation's
        assert np.array_equal(q["desc"], rg.desc[want["best_slot"]][want["best_index"]])
    else:
        assert (q["desc"] == 0xa5).all()
    if want["status"] & 1:
        assert q["max_distance"] == want["max_distance"] and q["min_distance"] == want["min_distance"] and q["min_distance"] < q["max_distance"]
    else:
        assert q["min_distance"] == np.float32(0.25) and q["max_distance"] == np.float32(64)


def test_every_mutant_has_a_case():
    assert set(m for c in S.CASES.values() for m in c["mutants"]) == set(P.MUTANTS)


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_mutant_changes_its_cases_and_only_them(mutant):
    changed = []
    for name, c in S.CASES.items():
        a, b = S.planted_graph(), S.planted_graph()
        if not (same(one(a, c["p"]), one(b, c["p"], mutant=mutant)) and S.state(a) == S.state(b)):
            changed.append(name)
    assert changed == [n for n, c in S.CASES.items() if mutant in c["mutants"]], (mutant, changed)


def test_what_selects_the_function():
    for name, c in S.CASES.items():
        full = one(S.planted_graph(), c["p"], 3)
        rg = S.planted_graph()
        d, s = one(rg, c["p"], 1), one(S.planted_graph(), c["p"], 2)
        assert d["status"] == full["status"] & 1 and s["status"] == full["status"] & 2, name
        assert d["min_distance"] == full["min_distance"] and d["best_slot"] == -1 and s["best_slot"] == full["best_slot"] and s["max_distance"] == 0
        assert (rg.point(c["p"])["desc"] == 0xa5).all(), name              # what = 1 leaves the descriptor alone


def test_select_and_ids_outside_the_map():
    rg = S.planted_graph()
    ids = [0, 7, -1, 99, 0, 20]
    out = P.refresh_points(rg, ids, 3, select=[1, 0, 1, 1, 1, 1], select_value=1)
    assert out["status"].tolist() == [3, 0, 0, 0, 3, 0] and out["best_slot"].tolist() == [1, -1, -1, -1, 1, -1]
    assert S.state(rg, [7]) == S.state(S.planted_graph(), [7])


def test_restatement_equals_the_sort_the_row_form_on_the_random_graph():
    rg = S.shapes_graph()
    g = rg.g
    seen_tie, seen_rest, n = 0, 0, 0
    for p in range(g.capacity):
        got = P.distinctive(rg, p)
        rows = [(s, i) for s, i in zip(g.obs[p], rg.obs_idx[p]) if not g.kf_bad[s] and 0 <= i < len(rg.desc[s])]
        if not rows:
            assert got is None
            continue
        pos, median = P.brute_force_descriptor([rg.desc[s][i] for s, i in rows], [g.mn_id[s] for s, _ in rows])
        assert got == (rows[pos][0], rows[pos][1], median), p
        n += 1
        seen_rest += len(g.obs[p]) > 64
        D = [[P.hamming(rg.desc[a][i], rg.desc[b][j]) for b, j in rows] for a, i in rows]
        meds = sorted(sorted(r)[int(0.5 * (len(rows) - 1))] for r in D)
        seen_tie += len(meds) > 1 and meds[0] == meds[1]
    assert n > 60 and seen_tie > 20 and seen_rest == 2                   # the graph exercises what it is for


def test_the_shapes_are_the_ones_named():
    rg = S.shapes_graph()
    assert [len(rg.g.obs[p]) for p in range(len(S.OBSERVER_COUNTS))] == list(S.OBSERVER_COUNTS)
    assert (rg.g.kf_capacity, rg.kf_stride, rg.obs_stride, rg.n_levels) == (140, 40, 160, 8)
    out = P.refresh_points(rg, np.arange(rg.g.capacity), 3)
    assert set(out["status"].tolist()) == {0, 1, 2, 3}                   # every combination occurs
    assert out["status"][0] == 0 and (out["status"][1:len(S.OBSERVER_COUNTS)] != 0).all()


def test_depth_is_binary32_and_ordered_as_pinned():
    """(x x + y y) + z z with every operation rounded once: a position where the other association gives another float"""
    pos, c = np.array([1e-3, 3.0, 4.0], np.float32), np.zeros(3, np.float32)
    d = P.point_distance(pos, c)
    assert d.dtype == np.float32 and d == np.float32(np.sqrt(np.float32(np.float32(np.float32(1e-3) ** 2 + np.float32(9)) + np.float32(16))))
