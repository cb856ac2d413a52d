"""A small map-graph model of the first loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:819-824): the current key
frame's map points are fused into K neighbours one after the other (ORBmatcher::Fuse, src/ORBmatcher.cc:678-851), and between two
searches the graph changes -- MapPoint::Replace makes one point bad and hands its observations to the survivor, whose descriptor
is recomputed (ComputeDistinctiveDescriptors, through the oracle); AddObservation puts a point into the key frame.

Two drivers over the same model:
  sequential(...)  K searches, each on the state of its moment, with the edits between them -- the truth;
  replay(...)      ONE search of all K targets on the state at the START of the loop, then the same walk: pairs that are skipped
                   by now are masked, points whose descriptor differs from the start-of-loop bytes ("dirty") get their result for
                   this target from `resolve`, every other pair takes the start-of-loop row.
The searches are pluggable, so the replay runs with the oracle alone (tests/test_neighbors_model.py) or with the library's batch
call, host selects and fallbacks (tests/test_fuse_neighbors_gpu.py)."""
import numpy as np

import frustum_scenarios as FS
import match_scenarios as S
import oracle_py as O
import test_fuse as TF
from test_frustum import ON

W, H, ARGS = TF.W, TF.H, TF.ARGS
TH_LOW = 50
SCENES = {  # the two scenes of the design note: observations of the targets' own points, share of our points already in a target
    "default": dict(fobs=(1, 6), inkf=0.3),
    "sparse": dict(fobs=(6, 11), inkf=0.8),
}


class MP:
    """what the loop reads and edits of a MapPoint: descriptor, the observed descriptors it is the median of, bad flag, the key
    frames it is observed in; slot = its entry in the id list (-1: a neighbour's own point)"""

    def __init__(self, desc, obs_descs, slot=-1):
        self.desc = desc.copy()
        self.set = [d.copy() for d in obs_descs]
        self.bad = False
        self.slot = slot
        self.kfs = set()

    def obs(self):
        return len(self.set)

    def recompute(self):  # MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:343-416)
        bi, _ = O.distinctive_descriptors(np.array([0, len(self.set)], np.int32), np.stack(self.set))
        self.desc = self.set[int(bi[0])].copy()


def replace(a, b, feat_mp):
    """a->Replace(b): a goes bad, b takes over a's observations and recomputes its descriptor (src/MapPoint.cc:262-314)"""
    a.bad = True
    b.kfs |= a.kfs
    for key, q in list(feat_mp.items()):
        if q is a:
            feat_mp[key] = b
    b.set += a.set
    a.set = []
    b.recompute()


def scene(seed=5, K=20, M=1200):
    """K neighbours built like tests/test_fuse_keyframe_gpu.py::test_search_in_neighbors_sequence: one scene seen again and
    again -- features shuffled, moved by a fraction of a pixel, a few descriptor bits flipped, some features missing"""
    from orbfe import synth
    eo = O.Extractor(*ARGS)
    kp0, desc0, _ = eo.extract(synth.frame(W, H, 90))
    rng = np.random.default_rng(seed)
    Fo = O.Frustum()
    v0 = FS.fill_frustum(Fo, ON, seed=60)
    pts, mpd, _, inv_s2 = TF.scenario(kp0, desc0, eo.scaleFactors, v0, M, 3, False)
    pts["skip"] = 0
    nbs = []
    for k in range(K):
        perm = rng.permutation(len(kp0))[:len(kp0) - 10 * k]
        kpk = kp0[perm].copy()
        kpk["x"] += rng.normal(0, 0.3, len(kpk)).astype(np.float32)
        kpk["y"] += rng.normal(0, 0.3, len(kpk)).astype(np.float32)
        desck = np.stack([S.flip_bits(desc0[i], int(rng.integers(0, 12)), rng) for i in perm])
        fvo = O.make_frame_view(kpk, desck, 64, 48, 0.0, 0.0, float(W), float(H), eo.scaleFactors)
        nbs.append(dict(kp=kpk, desc=desck, fv=fvo))
    return dict(eo=eo, pts=pts, mpd=mpd, inv_s2=inv_s2, Fo=Fo, nbs=nbs, K=K, M=M, seed=seed)


def build_graph(sc, fobs=(1, 6), inkf=0.3):
    rng = np.random.default_rng(sc["seed"] + 1)
    pts, mpd, M = sc["pts"], sc["mpd"], sc["M"]
    mps = [MP(mpd[i], [S.flip_bits(mpd[i], int(rng.integers(0, 8)), rng) for _ in range(int(rng.integers(2, 5)))], i) for i in range(M)]
    for p in mps:
        p.bad = bool(pts["bad"][p.slot])
    feat_mp = {}
    for k, nb in enumerate(sc["nbs"]):
        n = len(nb["kp"])
        for f in np.flatnonzero(rng.random(n) < 0.5):  # half of the neighbour's features carry a map point of its own
            q = MP(nb["desc"][f], [S.flip_bits(nb["desc"][f], int(rng.integers(0, 8)), rng) for _ in range(int(rng.integers(*fobs)))])
            q.kfs.add(k)
            feat_mp[(k, int(f))] = q
        for i in np.flatnonzero(rng.random(M) < inkf):  # our point is already observed in this neighbour
            mps[i].kfs.add(k)
    return mps, feat_mp


def new_stats():
    return dict(bad=0, survive=0, dirty=0, added=0, fused=0)


def apply_edits(k, nb, mps, feat_mp, bi, bd, stats):
    """the edits of Fuse for target k in list order (:836-855); counts the points whose descriptor changed meanwhile"""
    before = [p.desc.copy() for p in mps]
    for i, p in enumerate(mps):
        if p.bad or k in p.kfs:
            continue
        if bd[i] > TH_LOW:
            continue
        f = int(bi[i])
        q = feat_mp.get((k, f))
        if q is not None:
            if not q.bad:
                if q.obs() > p.obs():
                    replace(p, q, feat_mp)
                    stats["bad"] += 1
                else:
                    replace(q, p, feat_mp)
                    stats["survive"] += 1
        else:
            p.set.append(nb["desc"][f].copy())
            p.kfs.add(k)
            feat_mp[(k, f)] = p
            stats["added"] += 1
        stats["fused"] += 1
    stats["dirty"] += sum(1 for i, p in enumerate(mps) if not p.bad and not np.array_equal(before[i], p.desc))


def call_points(sc, mps, k):
    """the orbfe_world_point records and descriptors of a search into target k on the graph as it is NOW"""
    call = sc["pts"].copy()
    call["skip"] = [k in p.kfs for p in mps]
    call["bad"] = [p.bad for p in mps]
    return call, np.stack([p.desc for p in mps])


def oracle_search(sc, th, mps, k, sel=None):
    call, mpd = call_points(sc, mps, k)
    if sel is not None:
        call, mpd = call[sel], mpd[sel]
    return O.fuse_search(sc["nbs"][k]["fv"], sc["inv_s2"], None, sc["Fo"], th, call, mpd)


def graph_state(mps):
    return [(p.bad, sorted(p.kfs), p.desc.tobytes()) for p in mps]


def sequential(sc, th, **graph_kw):
    """-> (per-target (bestIdx, bestDist), final graph, stats): K oracle searches with the edits between them"""
    mps, fm = build_graph(sc, **graph_kw)
    st, seq = new_stats(), []
    for k, nb in enumerate(sc["nbs"]):
        bi, bd = oracle_search(sc, th, mps, k)
        seq.append((bi.copy(), bd.copy()))
        apply_edits(k, nb, mps, fm, bi, bd, st)
    return seq, graph_state(mps), st


def replay(sc, th, search_all, resolve, **graph_kw):
    """search_all(mps) -> raw[k] = (bestIdx, bestDist) for all K targets on the start-of-loop state;
    resolve(k, dirty, mps) -> (bestIdx, bestDist) of the points `dirty` (indices) for target k under their descriptors of NOW.
    -> (per-target results as used, final graph, stats, counters)"""
    mps, fm = build_graph(sc, **graph_kw)
    start = [p.desc.copy() for p in mps]
    raw = search_all(mps)
    st, used = new_stats(), []
    cnt = dict(dirty_pairs=0, stale_differs=0, targets_with_dirty=0)
    for k, nb in enumerate(sc["nbs"]):
        bi, bd = raw[k][0].copy(), raw[k][1].copy()
        now_skip = np.array([p.bad or k in p.kfs for p in mps])
        bi[now_skip], bd[now_skip] = -1, 256
        dirty = np.array([i for i, p in enumerate(mps) if not now_skip[i] and not np.array_equal(start[i], p.desc)], np.int64)
        if len(dirty):
            a, b = resolve(k, dirty, mps)
            cnt["dirty_pairs"] += len(dirty)
            cnt["stale_differs"] += int(((bi[dirty] != a) | (bd[dirty] != b)).sum())
            cnt["targets_with_dirty"] += 1
            bi[dirty], bd[dirty] = a, b
        used.append((bi, bd))
        apply_edits(k, nb, mps, fm, bi, bd, st)
    return used, graph_state(mps), st, cnt
