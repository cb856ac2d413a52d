"""The vocabulary path against the reference's own Thirdparty/DBoW2, compiled into oracle/_ref/dbow2_ref (tests/dbow2_ref.py):
TemplatedVocabulary::loadFromTextFile / transform / saveToTextFile, FORB::distance and DUtils::Random::RandomInt as the reference
wrote them, not as this project restated them.  Every comparison is exact: word counts, BowVector doubles (through %a),
FeatureVector contents, distances, drawn indices.

Three stated departures shape the inputs:
  * the files handed to the reference end WITHOUT a newline: its `while(!f.eof())` loop turns a final newline into one more node
    under the root whose descriptor and leaf flag were never written.  Nothing here asserts what the reference does with one;
  * without early leaves the two FeatureVectors are equal; with them they may differ only for features whose leaf lies above
    level L - levelsup, where the reference's node id is an uninitialised variable (test_s7_is_confined);
  * k = 1 aborts in the reference's loader and is not compared."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dbow2_ref as R
import oracle_py as O
import vocab_synth as vs

N_FEATURES = 300


def special_trees():
    return [("root65", R.tree_root65(), 1), ("one17", R.tree_one17(), 2)]


def shape_trees():
    return [("k%d_L%d_up%d" % s, R.tree(s[0], s[1], seed=100 * s[0] + s[1], dup_p=(0.0, 0.2, 0.4)[i % 3], stop_p=(0.5, 0.05, 0.3)[i % 3]), s[2])
            for i, s in enumerate(R.SHAPES)]


def test_reference_alone_loads_a_root_with_65_children(tmp_path):
    """before anything is compared on it: the reference's loader takes 65 children under a header k = 20 (k only sizes a reserve())
    and writes the same tree back"""
    t = R.tree_root65()
    src = R.text(t)
    back = open(R.resave(tmp_path, src)).read().split("\n")
    want = src.split("\n")
    assert back[-1] == "" and len(back) - 1 == len(want) == len(t["parent"])
    assert sum(1 for l in back[1:-1] if l.split()[0] == "0") == 65
    assert [l.split()[:34] for l in back[1:-1]] == [l.split()[:34] for l in want[1:]]
    nw, _, _ = R.transform(tmp_path, src, vs.features_near(t, 10, seed=1), 0)
    assert nw == t["nWords"]


CPU_TREES = shape_trees() + special_trees()


@pytest.mark.parametrize("name,t,levelsup", CPU_TREES, ids=[c[0] for c in CPU_TREES])
def test_oracle_equals_reference(tmp_path, name, t, levelsup):
    """no early leaves, duplicate centres up to 40 % (first-minimum ties), stop words up to 50 %, all 6 scoring x 4 weighting types"""
    feats = vs.features_near(t, N_FEATURES, seed=5)
    if name in ("root65", "one17"):
        assert_last_child_is_reached(tmp_path, t, feats)
    triples = None
    for scoring, weighting in R.PAIRS:
        nw, bow, fv = R.transform(tmp_path, R.text(t, scoring, weighting), feats, levelsup)
        onw, obow, ofv, triples = R.ours(t, feats, levelsup, scoring, weighting, triples)
        what = "%s scoring %d weighting %d" % (name, scoring, weighting)
        assert nw == onw, what + ": word count"
        assert bow == obow, what + ": BowVector"
        assert list(fv.items()) == list(ofv.items()), what + ": FeatureVector"
        assert len(bow) > 10 and sum(len(v) for v in fv.values()) > N_FEATURES // 3, what + ": the case compares next to nothing"


def assert_last_child_is_reached(tmp_path, t, feats):
    """plants the centres of words below the widest node's last child (weight > 0: a stopped word enters no FeatureVector) as
    features 3.. and has the reference confirm that a descent passes that child (a duplicate sibling in front of it would take
    the features: the tree's seed is chosen so that there is none)"""
    last = R.widest_last_child(t)
    below, stack = [], [last]
    while stack:
        i = stack.pop()
        kids = t["childIdx"][t["childOff"][i]:t["childOff"][i + 1]]
        stack += [int(c) for c in kids]
        if len(kids) == 0 and t["weight"][i] > 0:
            below.append(i)
    assert below
    planted = list(range(3, 3 + min(4, len(below))))
    feats[planted] = t["nodeDesc"][below[:len(planted)]]
    _, _, fv = R.transform(tmp_path, R.text(t), feats, t["L"] - int(t["depth"][last]))
    assert set(planted) & set(fv.get(last, [])), "no planted feature passes node %d in the reference's descent" % last


def leaf_of_word(t):
    is_leaf = np.diff(t["childOff"]) == 0
    is_leaf[0] = False
    leaf = np.zeros(t["nWords"], np.int64)
    leaf[t["wordId"][is_leaf]] = np.flatnonzero(is_leaf)
    return leaf


@pytest.mark.parametrize("p", [0.08, 0.3])
@pytest.mark.parametrize("k,L", [(10, 4), (4, 5)])
@pytest.mark.parametrize("up", ["0", "1", "L-1"])
def test_s7_is_confined(tmp_path, k, L, p, up):
    """early leaves: the BowVector is still the reference's, and the FeatureVector differs from it only where S7 says it may --
    for features whose leaf lies above level L - levelsup.  At levelsup = L - 1 that level is 1 and no leaf lies above it: the set
    is empty by construction and the FeatureVectors must be equal; at levelsup 0 and 1 the set holds at least 20 features."""
    levelsup = {"0": 0, "1": 1, "L-1": L - 1}[up]
    t = R.tree(k, L, seed=7 * k + L, early_leaf_p=p, dup_p=0.2, stop_p=0.1)
    leaf = leaf_of_word(t)
    # 300 features spread over the tree + 60 next to early leaves that carry a weight, so that the set is well filled
    early = np.flatnonzero((np.diff(t["childOff"]) == 0) & (t["depth"] < L - 1) & (t["weight"] > 0))
    assert len(early) > 0
    rng = np.random.default_rng(11)
    near = t["nodeDesc"][early[rng.integers(0, len(early), 60)]].copy()
    near[np.arange(60), rng.integers(0, 32, 60)] ^= np.uint8(1) << rng.integers(0, 8, 60).astype(np.uint8)
    feats = np.concatenate([vs.features_near(t, N_FEATURES, seed=7), near])
    nw, bow, fv = R.transform(tmp_path, R.text(t), feats, levelsup)
    onw, obow, ofv, (word, _, weight) = R.ours(t, feats, levelsup, 0, 0)
    assert nw == onw and bow == obow
    s7 = (t["depth"][leaf[word]] < L - levelsup) & (weight > 0)
    node_r, node_o = R.node_of(fv, len(feats)), R.node_of(ofv, len(feats))
    assert np.array_equal(node_r >= 0, node_o >= 0)  # the same features take part
    differs = node_r != node_o
    print("S7 set %d features, %d of them differ" % (s7.sum(), differs.sum()))
    assert not (differs & ~s7).any(), "features outside S7's set got another node than the reference's: %s" % np.flatnonzero(differs & ~s7)[:10]
    if levelsup == L - 1:
        assert not s7.any() and list(fv.items()) == list(ofv.items())
    else:
        assert s7.sum() >= 20
        assert (node_o[s7] == leaf[word][s7]).all()  # S7: the leaf's own id


def test_text_loader_ignores_the_final_newline(tmp_path):
    import orbfe
    t = R.tree(6, 3, seed=3, early_leaf_p=0.1)
    tabs = []
    for nl in (False, True):
        p = tmp_path / ("voc%d.txt" % nl)
        p.write_text(R.text(t, 2, 1, final_newline=nl))
        tabs.append(orbfe.load_vocabulary_text(str(p)))
    for key in ("k", "L", "scoring", "weighting"):
        assert tabs[0][key] == tabs[1][key]
    for key in ("childOff", "childIdx", "nodeDesc", "wordId", "weight"):
        assert np.array_equal(tabs[0][key], tabs[1][key]) and np.array_equal(tabs[0][key], t[key]), key


def test_text_loader_reads_what_the_reference_saves(tmp_path):
    """loadFromTextFile -> saveToTextFile by the reference, then our loader: the tables of the tree that was written.  saveToTextFile
    prints weights with 6 significant digits, so the tree's weights are rounded to 4 first (nothing else would survive it)."""
    import orbfe
    for t in (R.tree(6, 3, seed=3, early_leaf_p=0.1), R.tree_root65()):
        t["weight"] = np.array([float("%.4g" % w) for w in t["weight"]])
        out = R.resave(tmp_path, R.text(t, 1, 3))
        assert open(out).read().endswith("\n")  # as ORBvoc.txt does
        v = orbfe.load_vocabulary_text(out)
        assert (v["k"], v["L"], v["scoring"], v["weighting"]) == (t["k"], t["L"], 1, 3)
        for key in ("childOff", "childIdx", "nodeDesc", "wordId", "weight"):
            assert np.array_equal(v[key], t[key]), key


def test_forb_distance_equals_both_hammings(built, tmp_path):
    import orbfe
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (10000, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (10000, 32), dtype=np.uint8)
    b[:2000] = a[:2000] ^ (rng.random((2000, 32)) < 0.1).astype(np.uint8) * rng.integers(0, 256, (2000, 32), dtype=np.uint8)  # near pairs
    one = np.zeros((256, 32), np.uint8)  # every single bit of every byte
    one[np.arange(256), np.arange(256) // 8] = np.uint8(1) << (np.arange(256) % 8).astype(np.uint8)
    base = rng.integers(0, 256, (256, 32), dtype=np.uint8)
    a = np.concatenate([a, a[:4], a[4:8], base])
    b = np.concatenate([b, a[:4], ~a[4:8], base ^ one])
    ref = R.distance(tmp_path, a, b)
    assert len(ref) == len(a)
    assert (ref[10000:10004] == 0).all() and (ref[10004:10008] == 256).all() and (ref[10008:] == 1).all()
    assert np.array_equal(ref, np.unpackbits(a ^ b, axis=1).sum(axis=1))
    lib = np.array([orbfe.ORBmatcher.DescriptorDistance(a[i], b[i]) for i in range(len(a))])  # orbfe_hamming
    orc = np.array([O.hamming(a[i], b[i]) for i in range(len(a))])
    assert np.array_equal(lib, ref) and np.array_equal(orc, ref)


# ---- RandomInt: the min-sets of TwoViewReconstruction (8 of N) and MLPnPsolver (min_set of N)

def glibc_rand():
    libc = ctypes.CDLL(None)
    libc.srand(0)
    return libc.rand


def draw_from(randi, N, iterations, min_set):
    """the draw of src/TwoViewReconstruction.cc:75-94 / src/MLPnPsolver.cpp:121-141 on RandomInt results made elsewhere"""
    it_ = iter(randi)
    sets = np.zeros((iterations, min_set), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(min_set):
            r = next(it_)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def reference_sets(N, iterations, min_set):
    ds = [N - j for _ in range(iterations) for j in range(min_set)]
    randi = R.randomint(0, ds)  # SeedRandOnce(0), then RandomInt(0, d - 1) for the d of every draw
    assert len(randi) == len(ds) and all(0 <= r < d for r, d in zip(randi, ds))
    return draw_from(randi, N, iterations, min_set)


ITERATIONS = 40


@pytest.mark.parametrize("N", [8, 9, 20, 300])
def test_twoview_draw_sets_equal_reference_randomint(N):
    import twoview_ref
    assert np.array_equal(twoview_ref.draw_sets(N, ITERATIONS, glibc_rand()), reference_sets(N, ITERATIONS, 8))


@pytest.mark.parametrize("min_set", [6, 8])
@pytest.mark.parametrize("N", [8, 9, 20, 300])
def test_mlpnp_draw_sets_equal_reference_randomint(N, min_set):
    import mlpnp_ref
    assert np.array_equal(mlpnp_ref.draw_sets(N, ITERATIONS, min_set, glibc_rand()), reference_sets(N, ITERATIONS, min_set))


def program_sets(exe, args, min_set):
    out = subprocess.check_output([exe] + [str(a) for a in args]).decode()  # a fresh process: the stream starts at its seed
    return np.array([[int(x) for x in l.split()] for l in out.strip().split("\n")], np.int32).reshape(-1, min_set)


def test_adaptor_twoview_draw_sets_equal_reference_randomint(built):
    """TwoViewReconstruction::DrawSets of include/orbfe_adaptor.hpp (it seeds with srand(0) itself, once per process)"""
    import test_twoview_cpp as T
    exe = T._build()
    for N in (8, 9, 20, 300):
        assert np.array_equal(program_sets(exe, ["drawsets", N, ITERATIONS], 8), reference_sets(N, ITERATIONS, 8)), N


def test_adaptor_mlpnp_draw_sets_equal_reference_randomint(built):
    """MLPnPsolver::DrawSets of include/orbfe_adaptor.hpp (it never seeds, as the reference's does not: the program calls srand(0))"""
    import test_mlpnp_cpp as T
    exe = T._build()
    for N in (8, 9, 20, 300):
        for min_set in (6, 8):
            assert np.array_equal(program_sets(exe, ["drawsets", 0, N, ITERATIONS, min_set], min_set),
                                  reference_sets(N, ITERATIONS, min_set)), (N, min_set)


# ---- on the GPU: every expected value comes from oracle/_ref/dbow2_ref, fed the bytes the GPU sees

GPU_TREES = {  # name -> (tree, features per block of 256 threads, (weighting, scoring) besides the default)
    "k16": (lambda: R.tree(16, 3, seed=1603), 16, (1, 1)),
    "k17": (lambda: R.tree(17, 3, seed=1703), 4, (2, 0)),
    "k20": (lambda: R.tree(20, 3, seed=2003), 4, (3, 5)),
    "k2_L10": (lambda: R.tree(2, 10, seed=210), 16, (0, 5)),
    "root65": (R.tree_root65, 4, (1, 4)),
    "one17": (R.tree_one17, 4, (2, 2)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_TREES))
def test_gpu_transform_equals_reference(built, tmp_path, name):
    """vocab_transform_kernel at its own boundaries: maxChildren 16 | 17 (16-lane | 64-lane groups), a node with more children than
    the group has lanes (65: the second j += G pass), one 17-child node among 3-child ones, feature counts on both sides of a block's
    last group, levelsup on both sides of L; duplicate centres at 40 % so that the first minimum decides"""
    import orbfe
    make, per_block, pair = GPU_TREES[name]
    t = make()
    L = t["L"]
    assert int(np.diff(t["childOff"]).max()) > 16 if per_block == 4 else int(np.diff(t["childOff"]).max()) <= 16
    e = orbfe.ORBextractor(500, 2000, 1.2, 4, 20, 7, 320, 240)
    voc = orbfe.ORBVocabulary(e, t["childOff"], t["childIdx"], t["nodeDesc"], t["wordId"], t["weight"], L)
    all_feats = vs.features_near(t, 257, seed=9)
    if name in ("root65", "one17"):  # position 64 of 65 / 16 of 17: the lane that takes a second child
        assert_last_child_is_reached(tmp_path, t, all_feats)
        all_feats[0:3] = all_feats[3:6]  # also in the smallest launches
    sizes = (1, 15, 16, 17, 257) if per_block == 16 else (1, 3, 4, 5, 257)
    texts = {p: R.text(t, scoring=p[1], weighting=p[0]) for p in ((0, 0), pair)}
    compared = 0
    for n in sizes:
        for levelsup in (0, L - 1, L, L + 3):
            for weighting, scoring in ((0, 0), pair):
                nw, rbow, rfv = R.transform(tmp_path, texts[(weighting, scoring)], all_feats[:n], levelsup)
                bow, fv = voc.transform_bow(all_feats[:n], levelsup, weighting, scoring)
                what = "%s n=%d levelsup=%d weighting=%d scoring=%d" % (name, n, levelsup, weighting, scoring)
                assert nw == t["nWords"], what
                assert list(bow.items()) == rbow, what + ": BowVector"
                assert list(fv.items()) == list(rfv.items()), what + ": FeatureVector"
                compared += sum(len(v) for v in rfv.values())
    assert compared > 1000
    voc.close()


@pytest.mark.gpu
def test_gpu_chain_equals_reference(built, tmp_path):
    """orbfe_track_reference_keyframe on one 752 x 480 frame: the word / node / weight it returns assemble into the reference's
    BowVector and FeatureVector for the returned descriptors, and SearchByBoW on the reference's two FeatureVectors (key frame and
    frame) gives the chain's matches"""
    import orbfe
    from orbfe import synth
    from test_vocab import ref_bow
    cfg = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
    W, H, L, levelsup = 752, 480, 4, 2
    t = vs.spread_first_level(R.tree(10, L, seed=31, dup_p=0.05, stop_p=0.1), 32)
    txt = R.text(t)
    ex = orbfe.ORBextractor(*cfg)
    voc = orbfe.ORBVocabulary(ex, t["childOff"], t["childIdx"], t["nodeDesc"], t["wordId"], t["weight"], L)
    f1 = synth.frame(W, H, 640)
    kkp, kdesc = ex.extractFeatures(f1)  # the frame's own features as the key frame: most features find themselves
    _, _, kfv = R.transform(tmp_path, txt, kdesc, levelsup)
    knode = R.node_of(kfv, len(kkp)).astype(np.int32)
    kf = orbfe.KeyFrame(ex, kkp, kdesc, knode, ex.mvScaleFactor)
    has = np.ones(len(kkp), np.uint8)
    got = orbfe.FrameTracker(ex, 64, 48, 0.0, 0.0, float(W), float(H)).TrackReferenceKeyFrame(f1, voc, levelsup, kf, has, 0.75, True)
    nw, rbow, rfv = R.transform(tmp_path, txt, got["desc"], levelsup)
    bow, fv = ref_bow(got["word"], got["node"], got["weight"], 0, 0)
    assert nw == t["nWords"] and list(bow.items()) == rbow and list(fv.items()) == list(rfv.items())
    assert len(rbow) > 100 and len(rfv) > 20
    kfOff, kfIdx, fOff, fIdx = [0], [], [0], []
    for g in sorted(set(kfv) & set(rfv)):  # the lockstep walk of src/ORBmatcher.cc:150-165
        kfIdx += kfv[g]
        fIdx += rfv[g]
        kfOff.append(len(kfIdx))
        fOff.append(len(fIdx))
    n_b, match = O.search_by_bow(kfOff, kfIdx, fOff, fIdx, kdesc, kkp["angle"], has, got["desc"], got["kp"]["angle"], 0.75, True)
    assert got["nmatches"] == n_b and np.array_equal(got["match"], match)
    assert n_b > 200
    voc.close()


@pytest.mark.gpu
def test_gpu_adaptor_loader_equals_reference(built, tmp_path):
    """ORBVocabulary::loadFromTextFile of include/orbfe_adaptor.hpp uploads the tree, so it needs a handle: the file without and with
    the final newline, and the reference's own saveToTextFile output, must all transform like the reference"""
    import test_adaptor as A
    A._build()
    t = R.tree(6, 4, seed=64, early_leaf_p=0.0, dup_p=0.3)
    t["weight"] = np.array([float("%.4g" % w) for w in t["weight"]])  # survives saveToTextFile's 6 digits
    feats = vs.features_near(t, 200, seed=3)
    feats.tofile(str(tmp_path / "d.bin"))
    scoring, weighting = 1, 0
    want = R.transform(tmp_path, R.text(t, scoring, weighting), feats, 1)
    files = {"plain": R.text(t, scoring, weighting), "newline": R.text(t, scoring, weighting, final_newline=True),
             "resaved": open(R.resave(tmp_path, R.text(t, scoring, weighting))).read()}
    for name, txt in files.items():
        (tmp_path / "v.txt").write_text(txt)
        out = subprocess.check_output([A.BIN, "vocload", str(tmp_path / "v.txt"), str(tmp_path / "d.bin"), "1", str(tmp_path / "o.txt")]).decode()
        assert "vocload k=6 L=4 words=%d" % t["nWords"] in out, name
        got = R.parse_transform((tmp_path / "o.txt").read_text())
        assert got[0] == want[0] and got[1] == want[1] and list(got[2].items()) == list(want[2].items()), name
