"""tests/cpp/point_refresh.cpp: the program builds and links against the in-tree library; its plain C++ restatement of SPEC DECISION S26
on flat arrays -- with the arithmetic of csrc/spec_math.h and csrc/distinct_select.h, the texts the kernels compile -- equals
tests/point_refresh_ref.py on the scenes, output for output and record for record, without a GPU; on the GPU,
include/orbfe_adaptor.hpp's ResidentCovisibility::EnableRefresh / SetFeatures / SetCentres / SetObservations / SetReferenceKeyFrames /
RefreshPoints over mock KeyFrame / MapPoint objects give the same.  tests/cpp/point_refresh_check.cpp, the host-pure validation and
layout of the staged setters (csrc/covis_refresh_check.h), runs stand-alone under AddressSanitizer and UBSan on the CPU."""
import subprocess

import numpy as np
import pytest

import cpp_build
import point_refresh_ref as P
import point_refresh_scenarios as S


def _build():
    return cpp_build.build("point_refresh")


def test_point_refresh_program_builds_and_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


def test_setters_validation_and_layout_under_sanitizers(built):
    exe = cpp_build.build("point_refresh_check", san=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0 and "point_refresh_check: ok" in out and "FAIL" not in out, out


def _bits(a, dt):
    return np.ascontiguousarray(a, dt).view(np.int32).ravel().tolist()


def write_scene(path, rg, ids, what):
    g = rg.g
    w = [g.kf_capacity, g.capacity, rg.kf_stride, rg.obs_stride, rg.n_levels, len(ids), what] + _bits(rg.sf, np.float32)
    for s in range(g.kf_capacity):
        w += [int(g.is_set[s]), int(g.mn_id[s]), int(g.kf_bad[s]), len(rg.desc[s])] + [int(o) for o in rg.octave[s]]
        w += _bits(rg.desc[s], np.uint8) + _bits(rg.centre[s], np.float32)
    for p in range(g.capacity):
        w += [int(g.point_bad[p]), int(rg.ref[p]), len(g.obs[p])] + [int(s) for s in g.obs[p]] + [int(i) for i in rg.obs_idx[p]]
        w += _bits(rg.pos[p], np.float32) + _bits([rg.min_distance[p], rg.max_distance[p]], np.float32) + _bits(rg.map_desc[p], np.uint8)
    w += [int(i) for i in ids]
    np.array(w, np.int32).tofile(path)


def same(path, rg, ids, what, note):
    w = np.fromfile(path, np.int32)
    n, C = len(ids), rg.g.capacity
    assert len(w) == 6 * n + 10 * C
    rg = S.clone(rg)
    want = P.refresh_points(rg, ids, what)
    got = w[:6 * n].reshape(n, 6)
    for col, k in enumerate(("status", "min_distance", "max_distance", "best_slot", "best_index", "best_median")):
        assert np.array_equal(got[:, col], want[k].view(np.int32)), "%s: %s" % (note, k)
    rec = w[6 * n:].reshape(C, 10)
    assert np.array_equal(rec[:, 0], rg.min_distance.view(np.int32)) and np.array_equal(rec[:, 1], rg.max_distance.view(np.int32)), note
    assert np.array_equal(rec[:, 2:], rg.map_desc.view(np.int32)), note


def scenes():
    sh = S.shapes_graph()
    C = sh.g.capacity
    return dict(planted=(S.planted_graph(), S.PLANTED_IDS + [-1, 20, 16], 3), shapes=(sh, list(range(C)) + [8, 8, 3], 3),
                shapes_depth=(sh, list(range(C)), 1), shapes_descriptor=(sh, list(range(C)), 2))


@pytest.mark.parametrize("name", sorted(scenes()))
def test_host_restatement_equals_the_python_one(built, tmp_path, name):
    rg, ids, what = scenes()[name]
    write_scene(tmp_path / "scene.bin", rg, ids, what)
    subprocess.check_call([_build(), "host", str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")])
    same(tmp_path / "out.bin", rg, ids, what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("planted", "shapes"))
def test_adaptor_gives_the_restatements_records(built, tmp_path, name):
    rg, ids, what = scenes()[name]
    write_scene(tmp_path / "scene.bin", rg, ids, what)
    subprocess.check_call([_build(), "gpu", str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")])
    same(tmp_path / "out.bin", rg, ids, what, name + " through the adaptor")
