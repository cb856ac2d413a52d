"""The rotation-consistency filter of the matchers (rotation bin, ComputeThreeMaxima src/ORBmatcher.cc:1328-1370, drop
of the other bins) on CRAFTED histograms: random scenes rarely land on the edges -- ties under the strict ">", the
index shift chain, the binary32 10 % tests, the half-way and top-end inputs of roundf, the "+360" branch.

A profile is {bin: count}.  A scene realises it with one DESIGNATED pair per count -- identical descriptors, orientations
chosen for the bin -- among features whose descriptors are all more than 60 bits apart, so nothing else passes TH_LOW = 30.
Expected results are the C oracle's; each scene is first checked for validity on the oracle alone (no GPU)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb_slam3_v1.0_amd", "python"))  # when run as a script
import oracle_py as O  # noqa: E402

f32 = np.float32
HISTO = 30
EXTRA = 4  # features per side that belong to no designated pair

# name -> ({bin: count}, bins that survive the filter) -- the second column is written down by hand from :1328-1370
PROFILES = {
    "empty": ({}, set()),
    "single": ({12: 1}, {12}),
    "tie4": ({2: 3, 5: 3, 7: 3, 11: 3}, {2, 5, 7}),             # strict ">" keeps the first three
    "ascending": ({0: 1, 1: 2, 2: 3, 3: 4}, {3, 2, 1}),          # the index shift chain
    "descending": ({0: 4, 1: 3, 2: 2, 3: 1}, {0, 1, 2}),
    "second_at_10pct": ({4: 10, 9: 1}, {4, 9}),                  # f32(1) < f32(0.1) * f32(10) is false
    "second_below_10pct": ({4: 11, 9: 1}, {4}),                  # f32(1) < f32(0.1) * f32(11) is true
    "third_at_10pct": ({4: 10, 9: 5, 1: 1}, {4, 9, 1}),
    "third_below_10pct": ({4: 11, 9: 5, 1: 1}, {4, 9}),
}
HOST_ONLY = {"high_bins": ({13: 2, 20: 5, 29: 5, 17: 1, 25: 3}, {20, 29, 25})}  # raw bins the angles cannot reach

# explicit (angle1, angle2) pairs: rot = 0, 15, 45, 345, 359.99 -- the half-way and top-end inputs of roundf -- once with
# angle1 >= angle2 and once through the "+360" branch (angle1 < angle2)
EDGE_ROT = [0.0, 15.0, 45.0, 345.0, 359.99]
EDGE_ANGLES = [(r, 0.0) for r in EDGE_ROT] + [(f32(r) - f32(5.0), 355.0) for r in EDGE_ROT[1:]]


def rotation_bin_np(a1, a2):
    """:248-253 in binary32; roundf as floor(x + 0.5) on the non-negative product"""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0:
        rot = f32(rot + f32(360.0))
    b = int(np.floor(np.float64(f32(rot * f32(f32(1.0) / f32(HISTO)))) + 0.5))
    return 0 if b == HISTO else b


def three_maxima_np(hist):
    """:1328-1370: strict ">" and the two binary32 10 % tests"""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(hist):
        if s > m1:
            m3, m2, m1 = m2, m1, s
            i3, i2, i1 = i2, i1, i
        elif s > m2:
            m3, m2 = m2, s
            i3, i2 = i2, i
        elif s > m3:
            m3, i3 = s, i
    if f32(m2) < f32(f32(0.1) * f32(m1)):
        i2 = i3 = -1
    elif f32(m3) < f32(f32(0.1) * f32(m1)):
        i3 = -1
    return i1, i2, i3


def kept_bins(bins):
    hist = np.bincount(np.asarray(bins, np.int64), minlength=HISTO)
    return set(three_maxima_np(hist)) - {-1}


def angles_of(name):
    """-> (angle1[P], angle2[P], bin[P]) of the designated pairs of a case"""
    if name == "edges":
        a1 = np.array([a for a, _ in EDGE_ANGLES], f32)
        a2 = np.array([b for _, b in EDGE_ANGLES], f32)
    else:
        bins = [b for b, c in PROFILES[name][0].items() for _ in range(c)]
        # rot = 30 * bin exactly; every second pair of bins 1 .. 11 goes through the "+360" branch
        wrap = [k % 2 == 1 and 1 <= b <= 11 for k, b in enumerate(bins)]
        a1 = np.array([30.0 * b - 10.0 if w else 30.0 * b for b, w in zip(bins, wrap)], f32)
        a2 = np.array([350.0 if w else 0.0 for w in wrap], f32)
    got = np.array([rotation_bin_np(x, y) for x, y in zip(a1, a2)], np.int64)
    if name != "edges":
        assert got.tolist() == bins  # the angles realise the profile
    return a1, a2, got


CASES = list(PROFILES) + ["edges"]


@functools.lru_cache(maxsize=None)
def scene(name):
    """Both sides of a case: n = P + EXTRA features per side, pair k = (feature k, feature k) designated for k < P."""
    a1, a2, bins = angles_of(name)
    P = len(a1)
    n = P + EXTRA
    assert n <= 64
    rng = np.random.default_rng(1000 + CASES.index(name))
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d2[:P] = d1[:P]
    dist = np.unpackbits(d1[:, None, :] ^ d2[None, :, :], axis=2).sum(axis=2)
    des = np.zeros((n, n), bool)
    des[np.arange(P), np.arange(P)] = True
    assert (dist[des] == 0).all() and (dist[~des] > 60).all() and (dist[~des] < 256).all()
    for d in (d1, d2):  # ... and within a side as well
        own = np.unpackbits(d[:, None, :] ^ d[None, :, :], axis=2).sum(axis=2)
        assert (own[~np.eye(n, dtype=bool)] > 60).all()
    ang1 = np.concatenate([a1, rng.uniform(0, 360, EXTRA).astype(f32)])
    ang2 = np.concatenate([a2, rng.uniform(0, 360, EXTRA).astype(f32)])
    # level-0 keypoints at equal positions in both frames, 48 px apart in a 640 x 480 image
    kp1 = np.zeros(n, O.KP_DTYPE)
    kp1["x"] = 40.0 + 48.0 * (np.arange(n) % 12)
    kp1["y"] = 40.0 + 48.0 * (np.arange(n) // 12)
    kp1["size"] = 31.0
    kp2 = kp1.copy()
    kp1["angle"], kp2["angle"] = ang1, ang2
    expect_off = np.full(n, -1, np.int32)
    expect_off[:P] = np.arange(P)
    keep = kept_bins(bins)
    if name in PROFILES:
        assert keep == PROFILES[name][1]  # the restatement agrees with the hand-written column
    expect_on = np.where(np.isin(np.concatenate([bins, np.full(EXTRA, -1)]), sorted(keep)), expect_off, -1).astype(np.int32)
    return dict(P=P, n=n, kp1=kp1, kp2=kp2, d1=d1, d2=d2, bins=bins, keep=keep, expect={False: expect_off, True: expect_on})


W, H, SF = 640.0, 480.0, np.array([1.0, 1.2], f32)


def bow_args(S):
    """one key-frame feature and one frame feature per vocabulary node; the extras share one node (nothing matches there)"""
    P, n = S["P"], S["n"]
    off = list(range(P + 1)) + [n]
    idx = list(range(n))
    return (off, idx, off, idx, S["d1"], S["kp1"]["angle"], np.ones(n, np.uint8), S["d2"], S["kp2"]["angle"], 0.75)


def tri_args(S):
    """bCoarse: no epipolar geometry; the epipole is far from every keypoint (:551-565)"""
    P, n = S["P"], S["n"]
    off = list(range(P + 1)) + [n]
    idx = list(range(n))
    z = np.zeros(n, np.uint8)
    return (off, idx, off, idx, S["kp1"], S["d1"], z, None, S["kp2"], S["d2"], z, None, SF, np.eye(3, dtype=f32), (-1000.0, -1000.0),
            False, True)


def run_entry(entry, mod, matcher, S, check):
    """-> (nmatches, match vector) of one entry point; mod / matcher = orbfe and its ORBmatcher, or oracle_py and None"""
    if entry == "bow":
        # (SearchByBoW reports the key-frame feature per FRAME feature; pair k is (k, k), so the vector reads the same)
        return matcher.SearchByBoW(*bow_args(S), check) if matcher else O.search_by_bow(*bow_args(S), check)
    if entry == "tri":
        return matcher.SearchForTriangulation(*tri_args(S), check) if matcher else O.search_for_triangulation(*tri_args(S), check)
    f1 = mod.make_frame_view(S["kp1"], S["d1"], 64, 48, 0.0, 0.0, W, H, SF)
    f2 = mod.make_frame_view(S["kp2"], S["d2"], 64, 48, 0.0, 0.0, W, H, SF)
    return matcher.SearchForInitialization(f1, f2, 20, 0.9, check) if matcher else O.search_for_initialization(f1, f2, 20, 0.9, check)


ENTRIES = ["bow", "init", "tri"]


@functools.lru_cache(maxsize=None)
def oracle_result(entry, name, check):
    """The reference of a case, computed once; with the two validity conditions of the scene: check off -> exactly the
    designated pairs, check on -> exactly the designated pairs of the three_maxima bins of the intended profile."""
    S = scene(name)
    n, m = run_entry(entry, O, None, S, check)
    assert n == int((m >= 0).sum())
    assert np.array_equal(m, S["expect"][check]), (entry, name, check, m.tolist())
    return n, m


@pytest.mark.parametrize("entry", ENTRIES)
def test_scenes_are_valid_on_the_oracle(built, entry):
    for name in CASES:
        S = scene(name)
        n_off, m_off = oracle_result(entry, name, False)
        n_on, m_on = oracle_result(entry, name, True)
        assert n_off == S["P"]
        assert set(S["bins"][m_on[:S["P"]] >= 0].tolist()) == S["keep"], (entry, name)


def test_edge_rotations_reach_the_intended_bins():
    a1, a2, bins = angles_of("edges")
    assert bins.tolist() == [0, 1, 2, 12, 12, 1, 2, 12, 12]  # 0.5 -> 1, 1.5 -> 2, 11.5 -> 12, 11.9997 -> 12; never 30
    assert (a1[len(EDGE_ROT):] < a2[len(EDGE_ROT):]).all()


@pytest.mark.parametrize("check", [False, True])
def test_select_on_crafted_histograms_on_the_host(built, check):
    """orbfe_triangulation_select takes raw bins: every profile, one of bins 13 .. 29, plus entries that received a map
    point meanwhile (:506-509) and must not reach the histogram."""
    import orbfe
    for name, (profile, keep_by_hand) in list(PROFILES.items()) + list(HOST_ONLY.items()):
        bins = [b for b, c in profile.items() for _ in range(c)]
        top = max(profile, key=profile.get) if profile else 0
        # two entries of the fullest bin already hold a map point, two entries have no partner
        raw_bin = np.array(bins + [top, top, 0, 7], np.uint8)
        raw = np.concatenate([np.arange(len(bins)) + 100, [5, 6, -1, -1]]).astype(np.int32)
        now = np.array([0] * len(bins) + [1, 1, 0, 0], np.uint8)
        live = (raw >= 0) & (now == 0)
        keep = set(three_maxima_np(np.bincount(raw_bin[live].astype(np.int64), minlength=HISTO))) - {-1}
        assert keep == keep_by_hand, name
        want = np.where(live & (np.isin(raw_bin, sorted(keep)) if check else True), raw, -1)
        n, m12 = orbfe.triangulation_select(raw, raw_bin, now, check)
        assert n == int((want >= 0).sum()) and np.array_equal(m12, want), (name, check, m12.tolist())


@pytest.fixture(scope="module")
def matcher(built):
    import orbfe
    ex = orbfe.ORBextractor(300, 20000, 1.2, 2, 20, 7, int(W), int(H), device=0, max_batch=1)
    return orbfe.ORBmatcher(ex)


def _gpu_cases(orbfe, matcher, entries):
    for entry in entries:
        for name in CASES:
            for check in (False, True):
                n_ref, m_ref = oracle_result(entry, name, check)
                n, m = run_entry(entry, orbfe, matcher, scene(name), check)
                assert n == n_ref and np.array_equal(m, m_ref), (entry, name, check, m.tolist(), m_ref.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_crafted_histograms_hip_equals_oracle(built, matcher, entry):
    """SearchByBoW, SearchForInitialization (the two-phase kernel: these inputs are small) and SearchForTriangulation."""
    import orbfe
    _gpu_cases(orbfe, matcher, [entry])


@pytest.mark.gpu
def test_crafted_histograms_sequential_init_kernel(built):
    """SearchForInitialization's sequential kernel on the same scenes: forced by ORBFE_INIT_SLOW, which only the
    diagnostics build reads, in a child process that loads that build (as test_match_init.py does)."""
    import subprocess
    import __graft_entry__ as g
    g.build_variant("diag")
    env = dict(os.environ, ORBFE_INIT_SLOW="1", ORBFE_TEST_LIB="liborbfe_diag.so")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "forced sequential kernel: %d scenes exact" % len(CASES) in p.stdout, p.stdout[-1000:] + p.stderr[-2000:]


if __name__ == "__main__":  # child of test_crafted_histograms_sequential_init_kernel
    import orbfe
    orbfe.LIB_PATH = os.path.join(orbfe.CSRC, os.environ["ORBFE_TEST_LIB"])
    assert os.environ.get("ORBFE_INIT_SLOW") == "1"
    ex = orbfe.ORBextractor(300, 20000, 1.2, 2, 20, 7, int(W), int(H), device=0, max_batch=1)
    _gpu_cases(orbfe, orbfe.ORBmatcher(ex), ["init"])
    print("forced sequential kernel: %d scenes exact" % len(CASES))
