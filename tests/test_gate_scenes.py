"""CPU proof that the planted scenes of tests/gate_scenes.py are strong enough: every mutant of tests/gate_mutants.py -- one
gate of the oracle made wrong -- returns something else than the real oracle on at least one bare and one padded scene of its
function, in the arrays tests/test_gate_scenes_gpu.py compares.  A kernel with that mistake therefore fails the GPU test."""
import collections

import numpy as np
import pytest

import gate_mutants as GM
import gate_scenes as GS
import oracle_py as O


def same(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.fixture(scope="module")
def world(built):
    scenes = GS.scenes()
    real = [GS.run_oracle(s) for s in scenes]
    builder = GM.Builder()
    yield dict(scenes=scenes, real=real, builder=builder)
    builder.close()


def test_scale_tables_are_the_extractors(built):
    e = O.Extractor(1000, 40000, 1.2, GS.NLEVELS, 20, 7, 752, 480)
    assert e.scaleFactors.tobytes() == GS.SF.tobytes() and e.invLevelSigma2.tobytes() == GS.INV_S2.tobytes()


def test_scenes_are_deterministic(world):
    again = GS.scenes()
    assert [s["name"] + s["size"] for s in again] == [s["name"] + s["size"] for s in world["scenes"]]
    for s, t in zip(again, world["scenes"]):
        for k, v in s["args"].items():
            if isinstance(v, np.ndarray):
                assert v.tobytes() == t["args"][k].tobytes(), (s["name"], k)
        assert s["cases"], s["name"]
    covered = {s["matcher"] for s in again}
    for fn, matchers in GM.SCENES_OF.items():
        if any(m["fn"] == fn for m in GM.MUTANTS):
            assert covered & set(matchers), fn


# the sizes at which the kernels change path, as the code names them (csrc/match_proj.h, kernels_match_proj.hip, kernels_match_init.hip,
# kernels_match_bow.hip, match_proj.h): a padded scene that falls short of one of them leaves a kernel variant without the planted cases
K_RES_N_DESC, K_SORT_LDS, K_INIT_N, K_FAST_N0, K_BOW_NODE_CAP, K_RESOLVE_BATCHED_MIN = 1280, 2048, 2048, 1024, 512, 384
BARE_MAX = 300


def test_scene_sizes_reach_every_kernel_variant(world):
    by = collections.defaultdict(list)
    for s in world["scenes"]:
        by[s["matcher"]].append(s)
    for s in world["scenes"]:   # bare scenes are small
        if s["size"] == "bare":
            for k, v in s["args"].items():
                if isinstance(v, np.ndarray) and k in ("kp", "kp1", "kp2", "mps", "pts", "kfDesc", "fDesc"):
                    assert len(v) <= BARE_MAX, (s["name"], k, len(v))

    def frames(matcher, key="kp"):
        return sorted(len(s["args"][key]) for s in by[matcher])

    # frames of the window matchers: bare, above kResNDesc but within kResN, above kSortLds = kResN
    for matcher, key in (("projection", "kp"), ("fuse", "kp"), ("fuse_right", "kp"), ("fuse_sim3", "kp"), ("projection_kf", "kp"), ("sim3", "kp2")):
        n = frames(matcher, key)
        assert any(x <= BARE_MAX for x in n) and any(K_RES_N_DESC < x <= K_SORT_LDS for x in n) and any(x > K_SORT_LDS for x in n), (matcher, n)
    assert any(len(s["args"]["mps"]) > 256 for s in by["projection"]) and any(len(s["args"]["pts"]) > 256 for s in by["fuse"])
    assert GS.BATCHES[0] < 128 <= GS.BATCHES[1] < K_RESOLVE_BATCHED_MIN <= GS.BATCHES[2]
    # SearchForInitialization: the fast kernel, frame 1 with more than kFastN0 level-0 keypoints, frame 2 above kInitN
    shapes = [(int((s["args"]["kp1"]["octave"] == 0).sum()), len(s["args"]["kp2"])) for s in by["initialization"]]
    assert any(n0 <= K_FAST_N0 and n2 <= K_INIT_N for n0, n2 in shapes), shapes
    assert any(n0 > K_FAST_N0 and n2 <= K_INIT_N for n0, n2 in shapes), shapes
    assert any(n2 > K_INIT_N for n0, n2 in shapes) and any(n0 > K_SORT_LDS for n0, n2 in shapes), shapes
    # SearchByBoW: every node of a padded scene holds exactly the stated number of frame features; key-frame chunks of 64 and 65
    f_sizes, kf_sizes = set(), set()
    for s in by["bow"]:
        if s["size"] != "bare":
            f, k = np.diff(s["args"]["fOff"]), np.diff(s["args"]["kfOff"])
            assert f.min() == f.max(), (s["name"], s["size"])
            f_sizes.add(int(f[0]))
            kf_sizes |= {int(x) for x in np.unique(k)}
            assert s["args"]["nLeft"] == -1 or 0 < s["args"]["nLeft"] < len(s["args"]["fDesc"])
    assert {63, 64, 65, K_BOW_NODE_CAP, K_BOW_NODE_CAP + 1} <= f_sizes and {64, 65} <= kf_sizes, (f_sizes, kf_sizes)
    assert {-1} < {s["args"]["nLeft"] for s in by["bow"]}   # one camera and two
    # SearchForTriangulation: nodes of 64 and 65 key-frame-2 features
    t_sizes = {int(x) for s in by["triangulation"] if s["size"] != "bare" for x in np.unique(np.diff(s["args"]["off2"]))}
    assert {64, 65} <= t_sizes, t_sizes
    # isInFrustum: more points than one block takes
    assert max(len(s["args"]["pts"]) for s in by["frustum"]) > 4096
    # the candidate-sink crowd: exactly 16, exactly 17 and more
    for s in by["fuse"]:
        assert sorted(len(mine) for _, mine in s["crowd"]) == [16, 17, 24]


def test_control_build_equals_shipped_oracle(world):
    """the unmutated text built by the mutants' recipe == liborb_oracle.so on every planted scene"""
    with O.using(world["builder"].control()):
        for s, ref in zip(world["scenes"], world["real"]):
            assert same(GS.run_oracle(s), ref), (s["name"], s["size"])


def test_every_mutant_is_killed_bare_and_padded(world):
    mutants = GM.MUTANTS
    assert len({m["id"] for m in mutants}) == len(mutants)
    libs = world["builder"].build_all(mutants)
    survivors, not_equivalent = [], []
    for m in mutants:
        killed = collections.Counter()
        with O.using(libs[m["id"]]):
            for s, ref in zip(world["scenes"], world["real"]):
                if s["matcher"] in GM.SCENES_OF[m["fn"]] and not same(GS.run_oracle(s), ref):
                    killed["bare" if s["size"] == "bare" else "padded"] += 1
        if m["equivalent"]:
            if killed:
                not_equivalent.append("%s (%s -> %s)" % (m["id"], m["anchor"], m["repl"]))
        elif not (killed["bare"] and killed["padded"]):
            survivors.append("%s [%s -> %s] %s: killed on %d bare, %d padded scenes" % (m["id"], m["anchor"], m["repl"], m["what"],
                                                                                    killed["bare"], killed["padded"]))
    assert not survivors, "mutants the planted scenes cannot tell from the oracle:\n" + "\n".join(survivors)
    assert not not_equivalent, "marked equivalent but differing on a scene:\n" + "\n".join(not_equivalent)


def test_equivalents_are_few_and_argued():
    eq = [m for m in GM.MUTANTS if m["equivalent"]]
    assert 4 * len(eq) <= len(GM.MUTANTS), (len(eq), len(GM.MUTANTS))
    assert all(len(m["equivalent"]) > 40 for m in eq) and all(len(m["what"]) > 10 for m in GM.MUTANTS)
