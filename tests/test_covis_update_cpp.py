"""tests/cpp/covis_update.cpp: the program builds and links against the in-tree library; its plain C++ restatement of SPEC DECISION
S25 on flat arrays (the host side of the path tests/tools/covis_update_latency.py times) equals tests/covis_update_ref.py on the
scenes, output for output and key frame for key frame, without a GPU; and, on the GPU, include/orbfe_adaptor.hpp's
ResidentCovisibility::EnableConnections / AddKeyFrame / UpdateConnections over mock KeyFrame / MapPoint objects give the same."""
import subprocess

import numpy as np
import pytest

import covis_update_ref as U
import covis_update_scenarios as S
import cpp_build


def _build():
    return cpp_build.build("covis_update")


def test_covis_update_program_builds_and_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


def write_scene(path, sc):
    cg, g = sc.cg, sc.cg.g
    w = [g.kf_capacity, g.capacity, cg.kf_stride, cg.obs_stride, cg.child_stride, cg.conn_stride, len(sc.ops)]
    for s in range(g.kf_capacity):
        w += [int(g.is_set[s]), int(g.mn_id[s]), int(g.kf_bad[s]), int(g.parent[s]), int(g.prev[s]), len(g.points[s]), len(g.covisible[s]),
              len(g.children[s]), len(cg.conn[s])]
        w += [int(v) for v in g.points[s]] + list(g.covisible[s]) + list(g.children[s]) + [int(v) for kv in sorted(cg.conn[s].items()) for v in kv]
    w += [int(b) for b in g.point_bad]
    for o in g.obs:
        w += [len(o)] + list(o)
    for kind, a in sc.ops:
        if kind == "add":
            w += [0, a["slot"], a["mn_id"], int(a.get("bad", 0)), a.get("parent", -1), a.get("prev", -1), len(a["point_ids"])]
            w += [int(v) for v in a["point_ids"]]
        else:
            w += [1, len(a["slots"]), a.get("min_weight", U.MIN_WEIGHT)] + list(a["slots"]) + list(a["flags"])
    np.array(w, np.int32).tofile(path)


def read_results(path, sc):
    """-> (outputs per operation as Scene.trace gives them, key frames as ConnGraph.keyframe gives them, observation lists or None)"""
    w = np.fromfile(path, np.int32)
    at, outs, S_ = 0, [], sc.cg.conn_stride

    def take(n=None):
        nonlocal at
        if n is None:
            at += 1
            return int(w[at - 1])
        at += n
        return w[at - n:at]
    for kind, a in sc.ops:
        if kind == "add":
            n = take()
            outs.append(dict(added=take(n), status=take()))
        else:
            for _ in a["slots"]:
                count, status = take(), take()
                outs.append(dict(slots=take(S_), weights=take(S_), count=count, status=status))
    kfs = []
    for _ in range(sc.cg.g.kf_capacity):
        k = dict(mn_id=take(), bad=take(), parent=take(), prev=take(), n_features=take())
        k["covisible"] = take(take()).tolist()
        k["children"] = take(take()).tolist()
        pairs = take(2 * take()).tolist()
        k["conn"] = dict(zip(pairs[0::2], pairs[1::2]))
        kfs.append(k)
    obs = [take(take()).tolist() for _ in range(sc.cg.g.capacity)] if take() else None
    assert at == len(w)
    return outs, kfs, obs


def scenes():
    out = dict(S.gpu_scenes())
    out["observers_513"] = S.observers_scene(513)
    return out


def same(got, sc, what, adaptor=False):
    outs, kfs, obs = got
    want_outs, cg = sc.trace()
    assert len(outs) == len(want_outs)
    for k, (a, b) in enumerate(zip(outs, want_outs)):
        for name in b:
            assert np.array_equal(a[name], b[name]), "%s, output %d: %s\n%r\n%r" % (what, k, name, a[name], b[name])
    want = S.state(cg)
    for s, k in enumerate(kfs):
        assert k == want["kfs"][s], "%s: key frame %d\n%r\n%r" % (what, s, k, want["kfs"][s])
    if not adaptor:
        assert obs == want["obs"], what


@pytest.mark.parametrize("name", sorted(scenes()))
def test_host_restatement_equals_the_python_one(built, tmp_path, name):
    sc = scenes()[name]
    write_scene(tmp_path / "scene.bin", sc)
    subprocess.check_call([_build(), "host", str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")])
    same(read_results(tmp_path / "out.bin", sc), sc, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("threshold", "row_keeps_unconnected", "reciprocal_mixed", "sequence", "initialisation", "head_17", "no_counts"))
def test_adaptor_gives_the_restatements_graph(built, tmp_path, name):
    sc = scenes()[name]
    write_scene(tmp_path / "scene.bin", sc)
    subprocess.check_call([_build(), "gpu", str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")])
    same(read_results(tmp_path / "out.bin", sc), sc, name + " through the adaptor", adaptor=True)
