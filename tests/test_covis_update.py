"""tests/covis_update_ref.py, the normative restatement of SPEC DECISION S25, on its hand-written scenes: every scene gives what its
comment in tests/covis_update_scenarios.py works out by hand, and every mutant of the restatement changes the outputs of the scene
planted for it -- so the exact comparison of the GPU outputs with the restatement says something about each rule.  No GPU."""
import numpy as np
import pytest

import covis_update_ref as U
import covis_update_scenarios as S


def ordered(out):
    return [(int(s), int(w)) for s, w in zip(out["slots"][:out["count"]], out["weights"][:out["count"]])]


@pytest.mark.parametrize("name", sorted(S.planted_scenes()))
def test_planted_scene_gives_what_was_worked_out_by_hand(name):
    sc = S.planted_scenes()[name]
    outs, cg = sc.trace()
    e, g = sc.expect, cg.g
    last = outs[-1]
    if "ordered" in e:
        assert ordered(last) == e["ordered"] and last["status"] == U.OK
        assert (last["slots"][last["count"]:] == -1).all() and (last["weights"][last["count"]:] == 0).all()
    if "row" in e:
        assert cg.conn[sc.ops[-1][1]["slots"][-1]] == e["row"]
    if "row0" in e:
        assert cg.conn[0] == e["row0"]
    for s, head in e.get("head", {}).items():
        assert g.covisible[s] == head, (s, g.covisible[s])
    if "parent" in e:
        assert int(g.parent[2]) == e["parent"]
    for s, kids in e.get("children", {}).items():
        assert g.children[s] == kids
    if "added" in e:
        assert list(last["added"]) == e["added"] and last["status"] == U.OK
        assert list(g.points[2]) == [5, 5, 3, -1, 6, 99, 7] and not g.kf_bad[2] and g.mn_id[2] == 2
    for p, o in e.get("obs", {}).items():
        assert g.obs[p] == o


def test_every_mutant_has_a_scene():
    killed = set(m for sc in S.planted_scenes().values() for m in sc.kills)
    assert killed == set(U.MUTANTS)


@pytest.mark.parametrize("name,mutant", [(n, m) for n, sc in sorted(S.planted_scenes().items()) for m in sc.kills])
def test_mutant_changes_the_outputs_of_its_scene(name, mutant):
    sc = S.planted_scenes()[name]
    outs, cg = sc.trace()
    m_outs, m_cg = sc.trace(mutant=mutant)
    assert not (S.same_outputs(outs, m_outs) and S.state(cg) == S.state(m_cg)), "%s does not show in %s" % (mutant, name)


def test_threshold_mutant_shows_at_the_count_equal_to_min_weight():
    sc = S.planted_scenes()["threshold"]
    assert ordered(sc.trace(mutant="threshold_strict")[0][0]) == [(3, 51)]


def test_row_mutant_loses_the_unconnected_key_frame_from_the_head():
    _, cg = S.planted_scenes()["row_keeps_unconnected"].trace(mutant="own_row_connected_only")
    assert cg.g.covisible[0] == [1, 3]


def test_refusals_leave_the_graph_as_it_was():
    for name, sc in S.gpu_scenes().items():
        outs, cg = sc.trace()
        if any(o["status"] != U.OK for o in outs) and len(outs) == 1:
            assert S.state(cg) == S.state(sc.cg), name
            if "added" in outs[0]:
                assert not outs[0]["added"].any()
            else:
                assert outs[0]["count"] == 0 and (outs[0]["slots"] == -1).all()


def test_the_shapes_take_the_paths_they_are_named_for():
    sc = S.gpu_scenes()
    status = lambda n: [o["status"] for o in sc[n].trace()[0]]   # noqa: E731
    for what in ("neighbour_row", "children"):
        assert status("capacity_%s_-1" % what) == [U.OK] and status("capacity_%s_+0" % what) == [U.REFUSED], what
    assert [status("capacity_conn_stride_%+d" % d) for d in (-1, 0, 1)] == [[U.OK], [U.OK], [U.REFUSED]]   # conn_stride counts still fit
    assert status("capacity_neighbour_row_+1") == [U.OK]
    assert status("capacity_children_+1") == [U.OK]
    assert status("observation_list_-1") == [U.OK] and status("observation_list_+0") == [U.REFUSED] and status("observation_list_+1") == [U.OK]
    assert status("no_counts") == [U.NO_COUNTS]
    assert ordered(sc["double_slot"].trace()[0][0]) == [(1, 3)]
    assert ordered(sc["invalid"].trace()[0][0]) == [(3, 3), (1, 3)]
    for n, k in ((15, 15), (16, 16), (17, 16)):
        _, cg = sc["head_%d" % n].trace()
        assert len(cg.g.covisible[1]) == k and 0 in cg.conn[1] and not any(cg.g.kf_bad[c] for c in cg.g.covisible[1])
    outs, cg = sc["reciprocal_mixed"].trace()
    assert cg.g.covisible[1] == [0] and cg.g.covisible[2] == [4, 0] and cg.g.covisible[3] == [0, 1] and cg.conn[3][0] == 6
    outs, cg = sc["initialisation"].trace()
    assert [ordered(o) for o in outs] == [[(1, 100)], [(0, 100)]] and cg.g.parent[1] == 0 and cg.g.parent[0] == -1 and cg.g.children[0] == [1]
    for n in (512, 513):
        out = S.observers_scene(n).trace()[0][0]
        assert out["status"] == U.OK and out["count"] == sum(1 + k % 4 >= 3 for k in range(1, n + 1))
