"""tests/cpp/local_map.cpp: the program builds and links against the in-tree library; its plain C++ restatement of SPEC DECISION S24
on the flat arrays (the one-core yardstick of tests/tools/local_map_latency.py) equals tests/local_map_ref.py on the scenario files,
output for output, without a GPU; and, on the GPU, include/orbfe_adaptor.hpp's ResidentCovisibility + LocalMapUpdater over mock
KeyFrame / MapPoint objects give the same local key frames and id rows."""
import subprocess

import numpy as np
import pytest

import cpp_build
import local_map_ref as R
import local_map_scenarios as S


def _build():
    return cpp_build.build("local_map")


def test_local_map_program_builds_and_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


def write_scene(path, sc, **over):
    g, p = sc.g, {**sc.params, **over}
    w = [g.kf_capacity, g.capacity, sc.kf_stride, sc.obs_stride, sc.child_stride, len(sc.frames), sc.M, p["max_local_kf"], p["n_covisible"],
         p["n_temporal"], p["inertial"], p["mark_voters_seen"]]
    for s in range(g.kf_capacity):
        w += [int(g.is_set[s]), int(g.mn_id[s]), int(g.kf_bad[s]), int(g.parent[s]), int(g.prev[s]), len(g.points[s]), len(g.covisible[s]),
              len(g.children[s])]
        w += [int(v) for v in g.points[s]] + list(g.covisible[s]) + list(g.children[s])
    w += [int(b) for b in g.point_bad]
    for o in g.obs:
        w += [len(o)] + list(o)
    for votes, last in sc.frames:
        w += [len(votes), int(last)] + [int(v) for v in votes]
    np.array(w, np.int32).tofile(path)


def read_results(path, sc):
    w = np.fromfile(path, np.int32)
    at, out = 0, []
    for votes, _ in sc.frames:
        nk, npts = int(w[at]), int(w[at + 1])
        at += 2
        kfs = w[at:at + R.LOCAL_KF_MAX]
        at += R.LOCAL_KF_MAX
        ids = w[at:at + sc.M]
        at += sc.M
        n = int(w[at])
        at += 1
        out.append(dict(n_local_kfs=nk, n_local_points=npts, local_kfs=kfs, ids=ids, vote_ids=w[at:at + n]))
        at += n
        assert n == len(votes)
    assert at == len(w)
    return out


def scenes():
    out = dict(S.planted_scenes())
    out.update(random=S.random_scene(), random_marked=S.random_scene(seed=5, n_frames=6, mark_voters_seen=1, inertial=0),
               no_voters=S.no_voter_scene(), cut=S.truncation_scene(65, 64), walk=S.walk_scene(769, first_recurs_last=True),
               many_voted=S.vote_table_scene(513))
    return out


def same(got, want, what):
    for k in ("n_local_kfs", "n_local_points"):
        assert got[k] == want[k], "%s: %s %r != %r" % (what, k, got[k], want[k])
    for k in ("local_kfs", "ids", "vote_ids"):
        assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)


@pytest.mark.parametrize("name", sorted(scenes()))
def test_host_restatement_equals_the_python_one(built, tmp_path, name):
    sc = scenes()[name]
    write_scene(tmp_path / "scene.bin", sc)
    subprocess.check_call([_build(), "host", str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")])
    for f, got in enumerate(read_results(tmp_path / "out.bin", sc)):
        same(got, sc.ref(f), "%s, frame %d" % (name, f))


def test_time_mode_reports_a_figure(built, tmp_path):
    sc = S.planted_scenes()["parent_break"]
    write_scene(tmp_path / "scene.bin", sc)
    import json
    r = json.loads(subprocess.check_output([_build(), "time", str(tmp_path / "scene.bin"), "3"]).decode())
    assert r["host_ns_per_frame"] > 0 and r["frames"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("random", "random_marked", "parent_break", "no_voters"))
def test_adaptor_gives_the_restatements_local_map(built, tmp_path, name):
    sc = scenes()[name]
    g = sc.g
    for s in range(g.kf_capacity):                 # the adaptor lists the children in ascending mnId: the scene is given that order
        g.children[s] = sorted(g.children[s], key=lambda c: int(g.mn_id[c]))
    write_scene(tmp_path / "scene.bin", sc)
    subprocess.check_call([_build(), "gpu", str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")])
    for f, got in enumerate(read_results(tmp_path / "out.bin", sc)):
        want = sc.ref(f)
        v = np.asarray(sc.frames[f][0])
        want["vote_ids"] = np.where((v >= 0) & (v < g.capacity), want["vote_ids"], -1).astype(np.int32)   # outside the map: a null pointer
        # a feature slot that names an id outside the map is a null pointer to the adaptor: the same "no point"
        same(got, want, "%s through the adaptor, frame %d" % (name, f))
