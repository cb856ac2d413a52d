"""What the three per-frame chains (orbfe_track_frame, orbfe_track_reference_keyframe, orbfe_track_initialization) share on
the host and no other test reaches: the row-by-row re-pitch of a frame whose pitch is no multiple of four, in each chain,
and the bounded graph caches of the reference-key-frame chain (16 entries) and the initialisation chain (8 entries).  The
64-entry cache of orbfe_track_frame is covered in test_lifecycle_gpu.py."""
import numpy as np
import pytest

import frustum_scenarios as FS
import oracle_py as O
import vocab_synth as vs
from test_frustum import PN

pytestmark = pytest.mark.gpu

ARGS = (500, 20000, 1.2, 4, 20, 7, 320, 240)
W, H = ARGS[6], ARGS[7]
CHAINS = ("TrackFrame", "TrackReferenceKeyFrame", "TrackInitialization")


@pytest.fixture
def scene(built):
    """a fresh handle (its graph caches are empty), one frame, and what each chain runs against: map points on the frame's own
    keypoints, the frame's own features as reference key frame and as initial frame"""
    import orbfe
    from orbfe import synth
    img = synth.frame(W, H, 77)
    ex = orbfe.ORBextractor(*ARGS, device=0, max_batch=1)
    trk = orbfe.FrameTracker(ex, 16, 12, 0.0, 0.0, float(W), float(H))
    kp, desc = ex.extractFeatures(img)
    assert len(kp) > 100
    Fp = orbfe.Frustum()
    v = FS.fill_frustum(Fp, PN, W=float(W), H=float(H), n_levels=ARGS[3], seed=21)
    pts, mpd = FS.world_points_on_keypoints(kp.view(O.KP_DTYPE), desc, v, 400, np.random.default_rng(1), ARGS[3])
    pts = pts.view(orbfe.WP_DTYPE)
    t = vs.spread_first_level(vs.make_tree(8, 4, seed=2), 3)
    voc = orbfe.ORBVocabulary(ex, t["childOff"], t["childIdx"], t["nodeDesc"], t["wordId"], t["weight"], 4)
    _, node, weight = voc.transform(desc, 2)
    kf = orbfe.KeyFrame(ex, kp, desc, np.where(weight > 0, node, -1).astype(np.int32), ex.mvScaleFactor)
    has = np.ones(len(kp), np.uint8)
    ini = orbfe.InitialFrame(ex, kp, desc)

    def run(chain, src, nn=None):
        if chain == "TrackFrame":
            return trk.TrackFrame(src, Fp, pts, mpd, 20.0, 0.85 if nn is None else nn)
        if chain == "TrackReferenceKeyFrame":
            return trk.TrackReferenceKeyFrame(src, voc, 2, kf, has, 0.75 if nn is None else nn, True)
        return trk.TrackInitialization(src, ini, 40, 0.45 if nn is None else nn, True)

    yield dict(ex=ex, img=img, run=run)
    ini.close()
    kf.close()
    voc.close()
    ex.close()


def same_bytes(got, ref, what):
    assert got.keys() == ref.keys()
    for key in ref:
        if key == "nmatches":
            assert got[key] == ref[key], "%s: nmatches %d vs %d" % (what, got[key], ref[key])
        else:
            assert got[key].shape == ref[key].shape and got[key].tobytes() == ref[key].tobytes(), "%s: %s" % (what, key)


@pytest.mark.parametrize("chain", CHAINS)
def test_every_kind_of_source_gives_the_same_result(scene, chain):
    """The pageable packed frame (pitch 320: kept, one contiguous copy into the mirror) against a pageable frame of pitch 322
    (no multiple of four: re-pitched row by row into the mirror) and a pinned frame of pitch 336.  The staging rows of a
    320-wide handle are 320 bytes, so at this geometry the pinned padded frame is re-pitched as well; a pinned packed frame
    is added, the kind of source that is copied straight from the caller's buffer.  What is checked is that every source
    gives the same bytes and that no capture fails -- not which branch of the upload a source took: the results cannot tell."""
    import torch
    ex, img, run = scene["ex"], scene["img"], scene["run"]
    odd = np.zeros((H, W + 2), np.uint8)
    odd[:, :W] = img
    padded = torch.zeros((H, W + 16), dtype=torch.uint8).pin_memory().numpy()
    padded[:, :W] = img
    pinned = torch.from_numpy(img.copy()).pin_memory().numpy()
    assert odd[:, :W].strides[0] == W + 2 and padded[:, :W].strides[0] == W + 16 and pinned.strides[0] == W
    ref = run(chain, img)
    assert len(ref["kp"]) > 100 and ref["nmatches"] > 30
    same_bytes(run(chain, odd[:, :W]), ref, chain + ", pageable pitch %d" % (W + 2))
    same_bytes(run(chain, padded[:, :W]), ref, chain + ", pinned pitch %d" % (W + 16))
    same_bytes(run(chain, pinned), ref, chain + ", pinned packed")
    assert ex.graph_stats()[1] == 0


@pytest.mark.parametrize("chain,keys,bound", [("TrackReferenceKeyFrame", 20, 16), ("TrackInitialization", 10, 8)])
def test_bounded_graph_cache_is_dropped_and_refilled(scene, chain, keys, bound):
    """`keys` distinct ratios through a cache of `bound` graphs.  The cache drops everything when a new key finds `bound`
    entries, then takes the new one: every distinct key is captured exactly once on the way, the key that arrives at a full
    cache starts it afresh, so the last ratio is still cached afterwards and the first one is not.  Every fifth call equals
    the plain-launch path (stage timing on)."""
    ex, img, run = scene["ex"], scene["img"], scene["run"]
    assert bound < keys <= 2 * bound
    ratios = [0.60 + 0.01 * i for i in range(keys)]
    c0 = ex.graph_stats()[0]
    for i, nn in enumerate(ratios):
        got = run(chain, img, nn)
        if i % 5 == 0:
            ex.set_stage_timing(True)  # plain launches: no graph is looked up or captured
            plain = run(chain, img, nn)
            ex.set_stage_timing(False)
            same_bytes(got, plain, "%s, ratio %.2f" % (chain, nn))
    captured, failed = ex.graph_stats()
    assert captured - c0 == keys and failed == 0
    run(chain, img, ratios[-1])
    assert ex.graph_stats()[0] - c0 == keys, "the last ratio was captured again"
    run(chain, img, ratios[0])
    assert ex.graph_stats() == (c0 + keys + 1, 0), "the first ratio: dropped when key %d arrived, captured once more" % bound
