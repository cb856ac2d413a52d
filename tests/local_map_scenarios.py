"""Graphs and frames for the S24 tests (tests/local_map_ref.py): random line-shaped graphs, one planted scene per numbered rule of S24,
and the shapes at which the kernels' mechanisms change path (walk lengths around the block size, truncation at M, the vote table's
switch count).  No orbfe import at module level: upload() takes the module."""
import numpy as np

import local_map_ref as R


class Scene:
    """a graph, the strides its resident copy needs, the frames (vote ids, last_kf) and the call's parameters"""

    def __init__(self, g, frames, M, kills=(), kf_stride=None, obs_stride=None, child_stride=None, expect=None, **params):
        self.g, self.frames, self.M, self.kills, self.expect = g, frames, int(M), tuple(kills), expect
        self.kf_stride = kf_stride or max(1, max(len(p) for p in g.points))
        self.obs_stride = obs_stride or max(1, max(len(o) for o in g.obs))
        self.child_stride = child_stride or max(1, max(len(c) for c in g.children))
        self.params = dict(max_local_kf=10, n_covisible=5, n_temporal=10, inertial=1, mark_voters_seen=0)
        self.params.update(params)

    def ref(self, f, mutant=None, **over):
        votes, last_kf = self.frames[f]
        return R.update_local_map(self.g, votes, last_kf, self.M, mutant=mutant, **{**self.params, **over})


def _observe(g, max_obs=None, rng=None):
    """GetObservations() of every point from the key frames' feature lists, in slot order (shuffled with rng), cut at max_obs"""
    g.obs = [[] for _ in range(g.capacity)]
    for s in range(g.kf_capacity):
        for p in sorted(set(int(p) for p in g.points[s] if 0 <= p < g.capacity)):
            g.obs[p].append(s)
    for p in range(g.capacity):
        if rng is not None:
            rng.shuffle(g.obs[p])
        if max_obs is not None:
            del g.obs[p][max_obs:]


def random_scene(seed=0, n_kf=60, kf_stride=300, n_points=6000, n_frames=20, n_voters=200, vote_stride=256, M=4096, window=500, **params):
    """a line-shaped graph: key frame k sees a window of the points that slides with k, its covisibles are ranked by shared points, its
    parent is one of the few key frames before it; slots are a permutation of the creation order and mn_id has gaps, so neither the
    slot order nor the creation index can stand in for mn_id"""
    rng = np.random.default_rng(seed)
    g = R.Graph(n_kf + 4, n_points)
    g.point_bad[:] = rng.random(n_points) < 0.03
    slot = rng.permutation(n_kf)
    mn = np.cumsum(rng.integers(1, 4, n_kf))
    pts, parent = [], []
    for k in range(n_kf):
        nf = kf_stride - int(rng.integers(0, 40))
        lo = k * (n_points - window) // n_kf
        p = rng.integers(lo, lo + window, nf).astype(np.int32)
        p[rng.random(nf) < 0.25] = -1
        p[rng.random(nf) < 0.01] = n_points + 7          # outside the map: no point
        pts.append(p)
        parent.append(-1 if k == 0 else int(rng.integers(max(0, k - 4), k)))
    sets = [set(int(x) for x in p if 0 <= x < n_points) for p in pts]
    for k in range(n_kf):
        shared = sorted(((len(sets[k] & sets[j]), j) for j in range(n_kf) if j != k and sets[k] & sets[j]), key=lambda t: (-t[0], t[1]))
        kids = [j for j in range(n_kf) if parent[j] == k]
        rng.shuffle(kids)
        g.set_keyframe(int(slot[k]), int(mn[k]), bad=rng.random() < 0.08, parent=-1 if parent[k] < 0 else int(slot[parent[k]]),
                       prev=-1 if k == 0 else int(slot[k - 1]), points=pts[k], covisible=[int(slot[j]) for _, j in shared[:12]],
                       children=[int(slot[j]) for j in kids])
    _observe(g, max_obs=16, rng=rng)
    frames = []
    for _ in range(n_frames):
        c = int(rng.integers(0, n_kf))
        pool = np.concatenate([pts[j] for j in range(max(0, c - 2), min(n_kf, c + 3))])
        v = rng.choice(pool, vote_stride).astype(np.int32)     # with its -1 and outside-the-map entries, and duplicates
        frames.append((v[:n_voters], int(slot[c]) if rng.random() < 0.9 else -1))
    return Scene(g, frames, M, kf_stride=kf_stride, obs_stride=16, child_stride=8, **params)


def _tiny(n_kf, capacity=64):
    g = R.Graph(n_kf, capacity)
    g.point_bad[:] = False
    return g


def planted_scenes():
    """name -> Scene with one frame, `expect` = (local key frames, emitted ids) worked out by hand, `kills` = the mutants of the rule.
    Key frame s holds the points 10 s .. 10 s + 2 unless the scene says otherwise; the voters are points 50 and up."""
    out = {}
    own = lambda s: [10 * s, 10 * s + 1, 10 * s + 2]   # noqa: E731

    # rule 1: point 50 sits at two keypoints and votes twice, so key frame 1 (two votes) outranks key frame 0 (one vote: point 51);
    # point 52 is bad: no vote for key frame 2, and its entry is cleared
    g = _tiny(3)
    for s in range(3):
        g.set_keyframe(s, s, points=own(s))
    g.obs[50], g.obs[51], g.obs[52] = [1], [0], [2]
    g.point_bad[52] = True
    out["double_vote"] = Scene(g, [([50, 51, 50, 52, -1, 99], -1)], 16, inertial=0, expect=([1, 0], own(0) + own(1)))

    # rule 2: counts 3, 2, 2, 2, 2, 1 with mn_id descending in the slot; the cut at 3 falls inside the four-way tie
    g = _tiny(6)
    for s in range(6):
        g.set_keyframe(s, 100 - s, points=own(s))
    g.obs[50] = [0, 1, 2, 3, 4, 5]
    g.obs[51] = [0, 1, 2, 3, 4]
    g.obs[52] = [0]
    out["tie_at_the_cut"] = Scene(g, [([50, 51, 52], -1)], 32, ("ties_descending_id",), max_local_kf=3, inertial=0,
                                  expect=([0, 4, 3], own(3) + own(4) + own(0)))

    # rule 3: ranks are key frame 0 (3 votes, bad), 1 (2 votes), 2 (1 vote); with two places the bad one uses the first
    g = _tiny(3)
    for s in range(3):
        g.set_keyframe(s, s, bad=s == 0, points=own(s))
    g.obs[50], g.obs[51], g.obs[52] = [0, 1, 2], [0, 1], [0]
    out["bad_kf_uses_its_place"] = Scene(g, [([50, 51, 52], -1)], 16, ("bad_kf_keeps_place_off",), max_local_kf=2, inertial=0,
                                         expect=([1], own(1)))

    # rule 4: first phase 0, 1.  Key frame 0: covisibles 1 (listed), 5 (bad), 2 -> 2; children 6 (bad), 3 -> 3; parent 4 is BAD and
    # is added all the same, and the break leaves the outer loop: key frame 1's covisible 7 is never looked at.  n_covisible = 3 ends
    # the covisibles of key frame 0 at 2: its fourth, 7, is outside the N.
    g = _tiny(8, capacity=128)
    for s in range(8):
        g.set_keyframe(s, s, bad=s in (4, 5, 6), points=own(s))
    g.set_keyframe(0, 0, parent=4, points=own(0), covisible=[1, 5, 2, 7], children=[6, 3])
    g.set_keyframe(1, 1, points=own(1), covisible=[7])
    g.obs[50], g.obs[51] = [0, 1], [0]
    out["parent_break"] = Scene(g, [([50, 51], -1)], 32, ("parent_continue",), n_covisible=3, inertial=0,
                                expect=([0, 1, 2, 3, 4], own(4) + own(3) + own(2) + own(1) + own(0)))

    # rule 5: last_kf = 2 (new) -> prev 0 (listed in the first phase): the chain stands still there and 3, 0's prev, is never reached
    g = _tiny(4)
    for s in range(4):
        g.set_keyframe(s, s, points=own(s))
    g.set_keyframe(2, 2, prev=0, points=own(2))
    g.set_keyframe(0, 0, prev=3, points=own(0))
    g.obs[50] = [0]
    out["temporal_stall"] = Scene(g, [([50], 2)], 16, ("temporal_advance",), expect=([0, 2], own(2) + own(0)))

    # rule 6: two local key frames, walked last first; point 7 is twice in key frame 1 (slots 0 and 3) and once more in key frame 0;
    # point 9 is bad, slot value -1 is empty, 64 is outside the map
    g = _tiny(2)
    g.set_keyframe(0, 0, points=[20, 7, 21])
    g.set_keyframe(1, 1, points=[7, 30, -1, 7, 9, 64, 31])
    g.point_bad[9] = True
    g.obs[50], g.obs[51] = [0, 1], [0]
    out["first_occurrence"] = Scene(g, [([50, 51], -1)], 16, ("forward_kf_order", "last_occurrence"), inertial=0,
                                    expect=([0, 1], [7, 30, 31, 20, 21]))
    return out


def walk_scene(W, first_recurs_last=False, per_kf=400):
    """a walk of exactly W feature slots, every slot a point of its own: ceil(W / per_kf) key frames (at least one), all voted for by
    point 0, ranked by mn_id.  first_recurs_last: the walk's last slot holds the point of its first slot again."""
    n_kf = max(1, -(-W // per_kf))
    g = R.Graph(n_kf, W + 2)
    g.point_bad[:] = False
    walk = np.arange(1, W + 1, dtype=np.int32)
    if first_recurs_last and W > 1:
        walk[-1] = walk[0]
    for k in range(n_kf):                       # the walk runs over the list in reverse: the LAST key frame holds its first slots
        g.set_keyframe(n_kf - 1 - k, n_kf - 1 - k, points=walk[k * per_kf:(k + 1) * per_kf])
    g.obs[0] = list(range(n_kf))
    return Scene(g, [([0], -1)], max(W, 1) + 3, kf_stride=per_kf, inertial=0)


def truncation_scene(unique, M):
    """`unique` distinct points (each of them twice in the walk) against a row of M"""
    g = R.Graph(2, unique + 2)
    g.point_bad[:] = False
    ids = np.arange(1, unique + 1, dtype=np.int32)
    g.set_keyframe(0, 0, points=ids[::-1])
    g.set_keyframe(1, 1, points=ids)
    g.obs[0] = [0, 1]
    return Scene(g, [([0], -1)], M, inertial=0)


def vote_table_scene(n_voted, max_local_kf=10):
    """n_voted key frames with one vote each (one point seen by all of them); mn_id runs against the slot, so the answer is the
    max_local_kf highest slots"""
    g = R.Graph(n_voted, 8 + 2 * n_voted)
    g.point_bad[:] = False
    for s in range(n_voted):
        g.set_keyframe(s, n_voted - s, points=[8 + 2 * s, 8 + 2 * s + 1])
    g.obs[0] = list(range(n_voted))
    return Scene(g, [([0], -1)], 64, max_local_kf=max_local_kf, inertial=0)


def no_voter_scene():
    """nobody votes (empty, bad and out-of-range entries only): frame 0 has a last key frame with a chain of three behind it"""
    g = _tiny(4)
    for s in range(4):
        g.set_keyframe(s, s, prev=s - 1, points=[10 * s, 10 * s + 1])
    g.point_bad[5] = True
    g.obs[5] = [0, 1]
    return Scene(g, [([-1, 5, 99], 3), ([-1, 5, 99], -1)], 16, n_temporal=3)


def upload(orbfe, ex, sc):
    """-> (MapPoints, Covisibility) holding the scene's graph"""
    g = sc.g
    mp = orbfe.MapPoints(ex, g.capacity)
    pts = np.zeros(g.capacity, orbfe.WP_DTYPE)
    pts["bad"] = g.point_bad
    pts["observations"] = [len(o) for o in g.obs]
    mp.update(np.arange(g.capacity), pts, np.zeros((g.capacity, 32), np.uint8))
    cv = orbfe.Covisibility(ex, mp, g.kf_capacity, sc.kf_stride, sc.obs_stride, sc.child_stride)
    cv.set_keyframes([g.record(s) for s in range(g.kf_capacity) if g.is_set[s]])
    cv.set_observations(*g.observations_csr([p for p in range(g.capacity) if g.obs[p]]))
    return mp, cv
