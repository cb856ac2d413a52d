"""SPEC DECISION S24 on the CPU: the restatement (tests/local_map_ref.py) against hand-written tiny graphs, one per numbered rule, and
the mutants of the restatement against the scenes the GPU tests compare on -- a scene that does not tell a mutant from the rule proves
nothing about that rule when the GPU output equals the restatement's."""
import numpy as np
import pytest

import local_map_ref as R
import local_map_scenarios as S

PLANTED = S.planted_scenes()


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_restatement_on_the_planted_scene(name):
    sc = PLANTED[name]
    got = sc.ref(0)
    kfs, ids = sc.expect
    assert got["n_local_kfs"] == len(kfs) and list(got["local_kfs"][:len(kfs)]) == kfs and (got["local_kfs"][len(kfs):] == -1).all()
    assert got["n_local_points"] == len(ids) and list(got["ids"][:len(ids)]) == ids and (got["ids"][len(ids):] == R.NO_POINT).all()


def test_votes_are_cleared_only_where_the_point_is_bad():
    sc = PLANTED["double_vote"]
    assert list(sc.ref(0)["vote_ids"]) == [50, 51, 50, -1, -1, 99]          # 52 is bad; -1 and 99 (outside the map) stay as they came
    # without the second vote of point 50 the two key frames tie at one vote and mn_id decides: the double vote is what ranks them
    g, (votes, last) = sc.g, sc.frames[0]
    once = R.update_local_map(g, [v for i, v in enumerate(votes) if i != 2], last, sc.M, **sc.params)
    assert list(once["local_kfs"][:2]) == [0, 1] and list(sc.ref(0)["local_kfs"][:2]) == [1, 0]


def test_mark_voters_seen_emits_the_voters_complemented():
    sc = PLANTED["first_occurrence"]
    g = sc.g
    g.obs[7] = [1]                                                             # point 7 is itself a voter's point
    got = R.update_local_map(g, [50, 7, 51], -1, sc.M, **{**sc.params, "mark_voters_seen": 1})
    assert list(got["ids"][:5]) == [~7, 30, 31, 20, 21] and got["ids"][5] == R.NO_POINT == ~(~R.NO_POINT) and ~R.NO_POINT < 0
    g.obs[7] = []


def test_bad_parent_is_added_and_covisibles_end_at_n():
    sc = PLANTED["parent_break"]
    assert sc.g.kf_bad[4] and 4 in sc.ref(0)["local_kfs"]
    assert 7 in sc.ref(0, n_covisible=4, mutant="parent_continue")["local_kfs"]
    wide = sc.ref(0, n_covisible=0)                                           # no covisible at all: child 3, parent 4, stop
    assert list(wide["local_kfs"][:wide["n_local_kfs"]]) == [0, 1, 3, 4]


def test_cyclic_prev_chain_costs_n_temporal_steps():
    g = S._tiny(2)
    g.set_keyframe(0, 0, prev=1, points=[1])
    g.set_keyframe(1, 1, prev=0, points=[2])
    got = R.update_local_map(g, [], 0, 8, n_temporal=32)
    assert list(got["local_kfs"][:got["n_local_kfs"]]) == [0, 1] and list(got["ids"][:2]) == [2, 1]


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_every_mutant_of_the_rule_changes_the_planted_scene(name):
    sc = PLANTED[name]
    want = sc.ref(0)["ids"]
    for m in sc.kills:
        assert not np.array_equal(sc.ref(0, mutant=m)["ids"], want), m


def test_every_mutant_has_a_planted_scene():
    assert sorted(m for sc in PLANTED.values() for m in sc.kills) == sorted(R.MUTANTS)


def test_mutants_on_the_random_scene():
    """the first four mutants change most frames of the random scene the GPU test uses; the planted scenes make it every one"""
    sc = S.random_scene()
    base = [sc.ref(f)["ids"] for f in range(len(sc.frames))]
    hits = {m: sum(not np.array_equal(sc.ref(f, mutant=m)["ids"], base[f]) for f in range(len(sc.frames))) for m in R.MUTANTS}
    print(hits)
    for m in ("forward_kf_order", "last_occurrence"):
        assert hits[m] == len(sc.frames), hits
    assert sum(hits[m] > 0 for m in R.MUTANTS) >= 4, hits
    counts = [sc.ref(f)["n_local_points"] for f in range(len(sc.frames))]
    assert min(counts) > 500 and max(counts) < sc.M, counts                   # the row is neither empty nor truncated


@pytest.mark.parametrize("W", [0, 1, 63, 64, 65, 1023, 1024, 1025, 3073])
def test_walk_scene_has_the_length_it_says(W):
    sc = S.walk_scene(W, first_recurs_last=W == 3073)
    got = sc.ref(0)
    assert sum(len(p) for p in sc.g.points) == W
    assert got["n_local_points"] == (W - 1 if W == 3073 else W) and list(got["ids"][:min(W, 3)]) == list(range(1, min(W, 3) + 1))


def test_truncation_and_vote_table_scenes():
    for unique in (63, 64, 65):
        got = S.truncation_scene(unique, 64).ref(0)
        assert got["n_local_points"] == unique and list(got["ids"][:min(unique, 64)]) == list(range(1, min(unique, 64) + 1))
    sc = S.vote_table_scene(513)
    got = sc.ref(0)
    assert list(got["local_kfs"][:10]) == list(range(512, 502, -1)) and got["n_local_kfs"] == 10
    a, b = S.no_voter_scene(), S.no_voter_scene()
    assert list(a.ref(0)["local_kfs"][:3]) == [3, 2, 1] and a.ref(0)["n_local_points"] == 6 and list(a.ref(0)["vote_ids"]) == [-1, -1, 99]
    assert b.ref(1)["n_local_kfs"] == 0 and a.ref(0, inertial=0)["n_local_points"] == 0 and (a.ref(0, inertial=0)["ids"] == R.NO_POINT).all()


def test_frame_points_statement():
    ids = np.array([5, ~6, 7, R.NO_POINT, 8], np.int32)
    match = np.array([0, 1, 2, 3, 4, -1, 9, 2], np.int32)
    outlier = np.array([0, 0, 1, 0, 0, 0, 0, 0], np.uint8)
    obs = np.array([1] * 8 + [0], np.int32)
    assert list(R.frame_points(ids, match, outlier, 7, obs, 9)) == [5, -1, -1, -1, -1, -1, -1, -1]
    obs[8] = 2
    assert list(R.frame_points(ids, match, outlier, 8, obs, 9)) == [5, -1, -1, -1, 8, -1, -1, 7]
