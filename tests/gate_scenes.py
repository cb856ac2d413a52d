"""Planted gate-boundary scenes for the matchers (helper module, not a test).

Every scene is built from explicit keypoints, descriptors, poses and points: no image, no extraction, no random numbers.
A scene is a dict: `matcher` (which oracle call / library calls take it), `name`, `size` ("bare" or "padded-<what>"), `args`
(exactly what the call takes) and `cases`: (index of the planted record, the gate it is aimed at).  tests/test_gate_scenes.py
proves on the CPU that the scenes tell every mutant of tests/gate_mutants.py from the real oracle; tests/test_gate_scenes_gpu.py
runs the library on them.

Geometry.  The image is [32, 544) x [16, 400) with a 64 x 48 grid, so a cell is 8 x 8 pixels and gridInvW = gridInvH = 0.125
exactly: cell numbers, window edges and the pinhole projection (fx = fy = 256, identity pose, z = 1) are exact in binary32 and
a planted "exactly on the bound" is exactly on it.  Planted cases sit on a lattice of sites 40 pixels apart (the widest window
used is under 22 pixels), so a case sees only its own keypoints.  Filler keypoints (padded sizes) lie in the strip
356 <= y < 389 that no planted window but the one at maxY reaches, with descriptors at distance >= 140 from every planted one;
the first planted keypoint stays keypoint 0, half of the filler follows it, so every other planted index moves."""
import numpy as np

import oracle_py as O

f32 = np.float32
COLS, ROWS = 64, 48
MINX, MAXX, MINY, MAXY = 32.0, 544.0, 16.0, 400.0
NLEVELS = 8
FX = FY = 256.0
CX, CY = 288.0, 208.0
TH_LOW, TH_HIGH = 30, 100


def scale_factors(n=NLEVELS, s=1.2):
    sf = [f32(1.0)]
    for _ in range(1, n):
        sf.append(f32(np.float64(sf[-1]) * np.float64(f32(s))))  # src/ORBextractor.cc:92-108: float *= double(float scaleFactor)
    return np.array(sf, np.float32)


SF_STORE = np.zeros(2 * NLEVELS, np.float32)   # the views hand over the first NLEVELS entries; the zeros behind them are never read by the
SF_STORE[:NLEVELS] = scale_factors()           # real oracle (a mutant that forgets the level clamp reads a radius of 0 there, not foreign memory)
SF = SF_STORE[:NLEVELS]
INV_S2 = (f32(1.0) / (SF * SF)).astype(np.float32)
LOG_SF = f32(O.spec_logf(f32(1.2)))  # log(mfScaleFactor) as the spec's own logf gives it: q(1.2) is then exactly 1


def nxt(x, n=1):
    """x moved n units in the last place (n < 0: downwards)"""
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf) if n > 0 else f32(-np.inf))
    return x


def site(k):
    """centre of lattice site k (12 columns x 7 rows): 40 pixels apart, on cell corners"""
    assert 0 <= k < 84
    return f32(MINX + 40 + 40 * (k % 12)), f32(MINY + 40 + 40 * (k // 12))


def inert_spot(j):
    """projection of the j-th inert point of a padded scene: 20 pixels from the nearest site centre in x and in y, where no
    planted keypoint is within reach of a level-0 window"""
    return f32(MINX + 60 + 40 * (j % 11)), f32(MINY + 60 + 40 * (j // 11 % 6))


def pattern(s):
    """256-bit descriptor with 64 ones, different for every s"""
    bits = np.zeros(256, np.uint8)
    bits[[(s * 37 + 4 * t + (t // 16)) % 256 for t in range(64)]] = 1
    return np.packbits(bits)


def flip(desc, start, d):
    """`desc` with the d bits start, start + 1, ... flipped: Hamming distance exactly d"""
    bits = np.unpackbits(desc)
    bits[[(start + t) % 256 for t in range(d)]] ^= 1
    return np.packbits(bits)


def offset_exact(u, r, sign):
    """(outer, inner): the first float x on the `sign` side of u with |fl(x - u)| >= r and its neighbour inside the window.
    Where r is a multiple of x's unit in the last place (r = 5 here) outer is at exactly r; elsewhere it is the float just
    beyond r."""
    u, r = f32(u), f32(r)
    x = nxt(f32(u + f32(sign) * r), -4 * sign)
    while abs(f32(x - u)) < r:
        x = nxt(x, sign)
    return x, nxt(x, -sign)


class Frame:
    """keypoints of one frame or key frame with the per-keypoint arrays the calls take"""

    def __init__(self):
        self.rows = []

    def add(self, x, y, octave, desc, angle=0.0, **extra):
        self.rows.append(dict(x=f32(x), y=f32(y), octave=int(octave), desc=np.asarray(desc, np.uint8), angle=f32(angle), **extra))
        return len(self.rows) - 1

    @staticmethod
    def filler(k, octave0=False, low=False):
        d = np.full(32, 0x00 if low else 0xFF, np.uint8)   # `low`: the other family, ~250 bits from the usual filler
        d[k % 32] ^= np.uint8(k % 251 & 0x1F)
        return dict(x=f32(MINX + 4 + (k * 7) % 500 + 0.25), y=f32(MINY + 340 + (k * 3) % 32 + 0.5),
                    octave=0 if (octave0 or k % 3) else 1 + k % 7, desc=d, angle=f32((k * 11) % 360))

    def build(self, pad=0, octave0=False, defaults=None, low=False):
        """(kp, desc, extras, index map): `pad` filler keypoints; the first planted keypoint stays keypoint 0 (index 0 is an edge of
        its own), half of the filler follows it, then the other planted keypoints, then the rest of the filler"""
        before = pad // 2
        rows = self.rows[:1] + [self.filler(k, octave0, low) for k in range(before)] + self.rows[1:] + [self.filler(k, octave0, low) for k in range(before, pad)]
        self.index = lambda j: j if j == 0 else before + j
        kp = np.zeros(len(rows), O.KP_DTYPE)
        for f in ("x", "y", "octave", "angle"):
            kp[f] = [r[f] for r in rows]
        kp["size"] = 31.0
        kp["response"] = 50
        desc = np.stack([r["desc"] for r in rows]) if rows else np.zeros((0, 32), np.uint8)
        extras = {k: np.array([r.get(k, v) for r in rows]) for k, v in (defaults or {}).items()}
        return kp, np.ascontiguousarray(desc), extras, self.index


def view(kp, desc):
    return O.make_frame_view(kp, desc, COLS, ROWS, MINX, MINY, MAXX, MAXY, SF)


# ======================================================================================================================
# ORBmatcher::SearchByProjection(Frame, map points): th = 2 so r = 2.5 * 2 * sf[level] (5 pixels at level 0), nnRatio 0.75
# ======================================================================================================================
PROJ_TH, PROJ_NN, PROJ_FAR = 2.0, 0.75, 10.0
BATCHES = (3, 130, 384)   # identical frames per orbfe_match_projection_batch_device call: wave top-K, thread top-K, batched resolve


def proj_radius(level, view_cos=1.0, th=PROJ_TH):
    r = f32(2.5) if np.float64(f32(view_cos)) > 0.998 else f32(4.0)
    r = f32(r * f32(th))
    return f32(r * SF[level])


def projection_scene(total=0, pad_points=0):
    """total: keypoints of the padded frame (0: bare)"""
    F, mps, mpd, cases = Frame(), [], [], []
    k = [0]

    def new_site():
        k[0] += 1
        return k[0] - 1

    def point(u, v, level, desc, gate, view_cos=1.0, depth=5.0, in_view=1, bad=0, obs=1):
        mps.append((f32(u), f32(v), f32(view_cos), f32(depth), level, in_view, bad, obs))
        mpd.append(desc)
        cases.append((len(mps) - 1, gate))
        return len(mps) - 1

    def kpt(x, y, octave, desc, obs=-1):
        return F.add(x, y, octave, desc, init_obs=obs)

    # --- Hamming ties: first and last cell of the window, level pair (lvl - 1, lvl) ---
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u - 7, v - 7, 1, flip(P, 0, 20)); kpt(u + 7, v + 7, 2, flip(P, 40, 20))   # r = 7.2: first cell and last cell
    point(u, v, 2, P, "tie in best between the first and the last cell, levels lvl-1 / lvl: the first visited wins")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u + 1, v, 2, flip(P, 0, 20)); kpt(u + 1.5, v, 1, flip(P, 40, 20))          # same cell: index order
    point(u, v, 2, P, "tie in best inside one cell: the lower index wins")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u - 6, v + 6, 2, flip(P, 0, 20)); kpt(u + 6, v - 6, 1, flip(P, 40, 20))    # cells (x0, y1) and (x1, y0)
    point(u, v, 2, P, "tie in best between cells (x0, y1) and (x1, y0): columns are walked before rows")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u, v, 3, flip(P, 0, 28)); kpt(u + 1, v, 3, flip(P, 40, 30)); kpt(u + 6, v, 2, flip(P, 80, 30))
    point(u, v, 3, P, "tie in second best: bestLevel2 stays with the first (same level as best: ratio 28 > 0.75 * 30 refuses)")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u, v, 3, flip(P, 0, 28)); kpt(u + 1, v, 2, flip(P, 40, 30)); kpt(u + 6, v, 3, flip(P, 80, 30))
    point(u, v, 3, P, "tie in second best, the first on the other level: the escape holds")
    # --- keypoint index / rounded cell: PosInGrid rounds ---
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u + 4.8, v, 1, flip(P, 0, 20)); kpt(u + 1.6, v, 2, flip(P, 40, 20))       # first: cell +1 by rounding (+0 by truncation)
    point(u, v, 2, P, "tie between a keypoint at 0.6 of a cell (rounds up) and a later one in the cell below: x")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u, v + 4.8, 1, flip(P, 0, 20)); kpt(u, v + 1.6, 2, flip(P, 40, 20))
    point(u, v, 2, P, "the same in y")
    # --- thresholds ---
    for d, gate in ((TH_HIGH, "single candidate at TH_HIGH: matched"), (TH_HIGH + 1, "single candidate at TH_HIGH + 1: refused")):
        s = new_site(); u, v = site(s); P = pattern(s)
        kpt(u + 1, v - 1, 1, flip(P, 0, d))
        point(u, v, 1, P, gate)
    for d1, d2, same, gate in ((30, 40, True, "ratio at float equality 30 == 0.75 * 40, same level: matched"),
                               (31, 40, True, "ratio just failed, same level: refused"),
                               (35, 40, False, "ratio failed but bestLevel != bestLevel2: matched"),
                               (29, 40, True, "ratio passed")):
        s = new_site(); u, v = site(s); P = pattern(s)
        kpt(u + 2, v, 2, flip(P, 0, d2)); kpt(u - 2, v, 2 if same else 1, flip(P, 60, d1))
        point(u, v, 2, P, gate)
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u - 2, v, 1, flip(P, 0, 40)); kpt(u + 2, v, 2, flip(P, 60, 35))
    point(u, v, 2, P, "the new best inherits nothing: bestLevel2 is the level of the dethroned best (1), not its own (2)")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u - 2, v, 1, flip(P, 0, 30)); kpt(u + 2, v, 2, flip(P, 60, 31))
    point(u, v, 2, P, "best on lvl - 1, second on lvl: levels come from the keypoints")
    # --- window: keypoints at exactly r and one unit inside, all four sides (level 0: r = 5, level 3: r = 8.64) ---
    for level in (0, 3):
        r = proj_radius(level)
        for axis in "xy":
            for sign in (1, -1):
                for which in (0, 1):
                    s = new_site(); u, v = site(s); P = pattern(s)
                    c = (u if axis == "x" else v)
                    pos = offset_exact(c, r, sign)[which]
                    kpt(pos if axis == "x" else u + 1, pos if axis == "y" else v - 1, level, flip(P, 0, 10))
                    point(u, v, level, P, "keypoint %s r in %s%s, level %d" % (("at or just beyond", "one unit inside")[which], "+-"[sign < 0], axis, level))
    # --- level pair ---
    for lvl, octv, gate in ((3, 1, "only lvl - 2: refused"), (3, 2, "only lvl - 1: matched"), (3, 3, "only lvl: matched"),
                            (3, 4, "only lvl + 1: refused"), (0, 1, "level 0 query, octave 1: refused"), (0, 0, "level 0 query, octave 0")):
        s = new_site(); u, v = site(s); P = pattern(s)
        kpt(u + 1, v + 1, octv, flip(P, 0, 10))
        point(u, v, lvl, P, gate)
    # --- cell range of the window ---
    s = new_site(); u, v = site(s); P = pattern(s)     # level 0, r = 5: (u - minX - r) / 8 = k + 0.375 -> low column k, keypoint at k + 0.45
    kpt(u + 8 - 4.4, v, 0, flip(P, 0, 10))
    point(u + 8, v, 0, P, "keypoint in the partly covered low column")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u, v + 8 - 4.4, 0, flip(P, 0, 10))
    point(u, v + 8, 0, P, "keypoint in the partly covered low row")
    s = new_site(); u, v = site(s); P = pattern(s)     # (u + r) / 8 = k + 0.875 -> high column k + 1, keypoint at k + 0.6 rounds to k + 1
    kpt(u + 2 + 2.8, v, 0, flip(P, 0, 10))
    point(u + 2, v, 0, P, "keypoint in the last column of the window")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u, v + 2 + 2.8, 0, flip(P, 0, 10))
    point(u, v + 2, 0, P, "keypoint in the last row of the window")
    s = new_site(); u, v = site(s); P = pattern(s)     # u + 5 - r == u: the low edge is exactly cell boundary k
    kpt(u + 5 - 4.5, v, 0, flip(P, 0, 10))
    point(u + 5, v, 0, P, "low window edge exactly on a cell boundary (x)")
    s = new_site(); u, v = site(s); P = pattern(s)     # u + 3 + r == u + 8: the high edge is exactly cell boundary k + 1
    kpt(u, v + 3 + 4.5, 0, flip(P, 0, 10))
    point(u, v + 3, 0, P, "high window edge exactly on a cell boundary (y)")
    # --- windows clipped at each image side, the last column / row being 0, and entirely outside ---
    P = pattern(50)
    kpt(MINX + 1, MINY + 100, 0, flip(P, 0, 10))
    point(MINX - 3, MINY + 100, 0, P, "window clipped at the left side")
    kpt(MINX - 1, MINY + 150, 0, flip(P, 0, 11))
    point(MINX - 5, MINY + 150, 0, P, "window whose last column is column 0 (u + r == minX)")
    kpt(MINX + 100.5, MINY + 1, 0, flip(P, 0, 12))
    point(MINX + 100.5, MINY - 3, 0, P, "window clipped at the top")
    kpt(MINX + 150.5, MINY - 1, 0, flip(P, 0, 13))
    point(MINX + 150.5, MINY - 5, 0, P, "window whose last row is row 0 (v + r == minY)")
    kpt(MAXX - 5.5, MINY + 200, 0, flip(P, 0, 14)); kpt(MAXX - 1, MINY + 200, 0, flip(P, 30, 5))
    point(MAXX - 2, MINY + 200, 0, P, "window clipped at the right side; the nearer keypoint rounds to column 64 == column 0 of the next row "
                                      "(PosInGrid checks the linear index only) and is never visited")
    kpt(MINX + 1, MINY + 1, 0, flip(P, 0, 16))
    point(MINX + 2, MINY + 2, 0, P, "keypoint in cell (0, 0)")
    point(MAXX + 9, MINY + 250, 0, P, "window entirely right of the grid")
    point(MINX - 14, MINY + 250, 0, P, "window entirely left of the grid")
    point(MINX + 250, MINY - 14, 0, P, "window entirely above the grid")
    point(MINX + 250, MAXY + 9, 0, P, "window entirely below the grid")
    # --- taken keypoints, claims, the point gates ---
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u + 1, v, 1, flip(P, 0, 5), obs=1); kpt(u - 1, v, 1, flip(P, 30, 50))
    point(u, v, 1, P, "the better keypoint holds a map point with 1 observation: skipped")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u + 1, v, 1, flip(P, 0, 5), obs=0); kpt(u - 1, v, 1, flip(P, 30, 50))
    point(u, v, 1, P, "the better keypoint holds a map point with 0 observations: not skipped")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u + 1, v, 1, flip(P, 0, 10)); kpt(u - 1, v, 1, flip(P, 30, 60))
    point(u, v, 1, P, "claims a keypoint, 2 observations", obs=2)
    point(u, v, 1, flip(P, 0, 5), "a later point nearer to the claimed keypoint: takes the other one")
    s = new_site(); u, v = site(s); P = pattern(s)
    kpt(u + 1, v, 1, flip(P, 0, 10)); kpt(u - 1, v, 1, flip(P, 30, 60))
    point(u, v, 1, P, "claims a keypoint, 0 observations", obs=0)
    point(u, v, 1, flip(P, 0, 5), "a later point overwrites the claim of a point with 0 observations")
    for kw, gate in ((dict(in_view=0), "not in view"), (dict(bad=1), "bad"), (dict(depth=PROJ_FAR), "depth exactly thFarPoints: kept"),
                     (dict(depth=nxt(PROJ_FAR)), "depth one unit beyond thFarPoints: dropped"),
                     (dict(view_cos=f32(0.998)), "viewCos == 0.998f is above the double 0.998: narrow radius, keypoint at 3 * th * sf outside"),
                     (dict(view_cos=nxt(0.998, -1)), "viewCos one unit below: wide radius")):
        s = new_site(); u, v = site(s); P = pattern(s)
        kpt(u + 6.5, v, 0, flip(P, 0, 10)) if "view_cos" in kw else kpt(u + 1, v, 0, flip(P, 0, 10))
        point(u, v, 0, P, gate, **kw)
    assert k[0] <= 84, k[0]

    # inert points of the padded sizes: not in view, or projecting where no keypoint is
    for j in range(pad_points):
        mps.append(inert_spot(j) + (f32(1), f32(5), 0, int(j % 3 != 0), 0, 1))
        mpd.append(pattern(100 + j))
    pad = max(0, total - len(F.rows))
    kp, desc, extras, _ = F.build(pad, defaults=dict(init_obs=-1))
    rec = np.array(mps, dtype=O.MP_DTYPE)
    return dict(matcher="projection", name="projection", size="bare" if not pad else "padded-%d" % len(kp), cases=cases,
                args=dict(kp=kp, desc=desc, mps=rec, mpDesc=np.ascontiguousarray(np.stack(mpd)), initObs=extras["init_obs"].astype(np.int32),
                          th=PROJ_TH, nnRatio=PROJ_NN, bFarPoints=True, thFarPoints=PROJ_FAR))


def oracle_projection(a):
    n, out = O.search_by_projection(view(a["kp"], a["desc"]), a["mps"], a["mpDesc"], a["initObs"], a["th"], a["nnRatio"],
                                    a["bFarPoints"], a["thFarPoints"])
    return dict(n=np.int64(n), match=out)


# ======================================================================================================================
# Camera of the projecting matchers: identity pose, pinhole, z = 1, so u = 256 x + 288 and v = 256 y + 208 exactly
# ======================================================================================================================
MBF = 47.9
FRUSTUM = dict(rcw=(1, 0, 0, 0, 1, 0, 0, 0, 1), tcw=(0, 0, 0), twc=(0, 0, 0), min_x=MINX, max_x=MAXX, min_y=MINY, max_y=MAXY, fx=FX, fy=FY,
               cx=CX, cy=CY, k1=0.0, k2=0.0, k3=0.0, k4=0.0, mbf=MBF, log_scale_factor=float(LOG_SF), n_levels=NLEVELS, camera_model=0)
ORACLE_NAMES = dict(rcw="rcw", tcw="tcw", twc="twc", min_x="minX", max_x="maxX", min_y="minY", max_y="maxY", fx="fx", fy="fy", cx="cx",
                    cy="cy", k1="k1", k2="k2", k3="k3", k4="k4", mbf="mbf", log_scale_factor="logScaleFactor", n_levels="nLevels",
                    camera_model="cameraModel")


def frustum(cls, names=None, v=FRUSTUM):
    """v as the oracle's struct (names = ORACLE_NAMES) or the library's (names = None: its fields carry v's names)"""
    F = cls()
    for k, x in v.items():
        f = names[k] if names else k
        if k in ("rcw", "tcw", "twc"):
            for i, y in enumerate(x):
                getattr(F, f)[i] = float(y)
        else:
            setattr(F, f, x)
    return F


def back_project(u, v, z=1.0):
    """(x, y, z) whose pinhole projection is exactly (u, v) in binary32"""
    x, y = f32(f32(f32(u) - f32(CX)) / f32(FX) * f32(z)), f32(f32(f32(v) - f32(CY)) / f32(FY) * f32(z))
    assert f32(f32(f32(FX) * x / f32(z)) + f32(CX)) == f32(u) and f32(f32(f32(FY) * y / f32(z)) + f32(CY)) == f32(v), (u, v)
    return x, y, f32(z)


def norm3(x, y, z):
    return f32(np.sqrt(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))))


def spec_q(max_d, dist):
    """the quotient PredictScale takes the ceiling of (S8)"""
    return f32(f32(O.spec_logf(f32(f32(max_d) / f32(dist)))) / LOG_SF)


def predict_level(max_d, dist):
    q = spec_q(max_d, dist)
    if not q > 0:
        return 0
    if q >= NLEVELS:
        return NLEVELS - 1
    return min(int(np.ceil(q)), NLEVELS - 1)


def max_distance_for(dist, level):
    """a maxDistance that puts the point in the middle of `level`"""
    m = f32(np.float64(dist) * 1.2 ** (level - 0.5))
    assert predict_level(m, dist) == level
    return m


_EDGE = {}


def level_edge(dist, k):
    """maxDistance values around dist * 1.2^k: (largest with q < k, all with q == k exactly, smallest with q > k), by search"""
    key = (float(dist), k)
    if key not in _EDGE:
        m = nxt(f32(np.float64(dist) * np.float64(f32(1.2)) ** k), -24)
        below, exact, above = None, [], None
        for _ in range(48):
            q = spec_q(m, dist)
            if q < k:
                below = m
            elif q == k:
                exact.append(m)
            elif above is None:
                above = m
            m = nxt(m)
        assert below is not None and above is not None
        _EDGE[key] = (below, exact, above)
    return _EDGE[key]


def scaled_bound(target, c):
    """d with fl(c * d) == target exactly (c = 0.9f or 1.1f), by search around target / c"""
    target, c = f32(target), f32(c)
    d = nxt(f32(target / c), -4)
    for _ in range(9):
        if f32(c * d) == target:
            return d
        d = nxt(d)
    raise AssertionError("no d with %r * d == %r" % (c, target))


def split_bound(u, v, c32, c64, up):
    """(x, y, z, d): a point within 1.5 pixels of (u, v) and a distance bound d with fl(c32 * d) == dist3D exactly while the double
    constant gives the neighbouring float (above dist3D if `up`, else below): only the float constant keeps the point"""
    for j in range(-12, 13):
        for i in range(-12, 13):
            x, y, z = back_project(f32(u + i / 8.0), f32(v + j / 8.0))
            dist = norm3(x, y, z)
            d = nxt(f32(dist / f32(c32)), -3)
            for _ in range(7):
                other = f32(np.float64(c64) * np.float64(d))
                if f32(f32(c32) * d) == dist and (other > dist if up else other < dist):
                    return x, y, z, d
                d = nxt(d)
    raise AssertionError("no split bound near (%r, %r)" % (u, v))


def chi2_values(unit, inv, target, n_terms):
    """(ex, ey, er) in multiples of `unit` with fl(fl(fl(ex^2 + ey^2) [+ er^2]) * inv) == target exactly, by search: for
    each of 40000 values of ey the three ex nearest to the real solution are tried"""
    target, inv = f32(target), f32(inv)
    goal2 = np.float64(target) / np.float64(inv)
    for er in ((f32(1.5), f32(1.25), f32(1.75), f32(1.375), f32(1.625)) if n_terms == 3 else (f32(0),)):
        ey = ((int(0.5 / unit) + np.arange(60000)) * np.float64(unit)).astype(np.float32)
        k0 = np.rint(np.sqrt(goal2 - ey.astype(np.float64) ** 2 - np.float64(er) ** 2) / unit)
        for dk in (0, -1, 1, -2, 2):
            ex = ((k0 + dk) * np.float64(unit)).astype(np.float32)
            e2 = ex * ex + ey * ey
            if n_terms == 3:
                e2 = e2 + f32(er * er)
            ok = (e2 * inv) == target
            if n_terms == 3:  # and the sum taken in the other order falls below the target: the order of the three squares matters here
                ok &= ((ex * ex + (ey * ey + f32(er * er))) * inv) < target
            hit = np.flatnonzero(ok)
            if len(hit):
                return f32(ex[hit[0]]), f32(ey[hit[0]]), er
    raise AssertionError("no chi-square value of exactly %r found" % target)


# ======================================================================================================================
# The search part of ORBmatcher::Fuse: fuse (mono and stereo key frame), fuse_right, fuse_sim3 on one set of planted cases
# ======================================================================================================================
FUSE_TH = 3.0


def fuse_world(pad=0, pad_points=0):
    F, pts, mpd, cases, crowd = Frame(), [], [], [], []
    k = [0]

    def new_site():
        k[0] += 1
        return site(k[0] - 1) + (pattern(k[0] - 1),)

    def point(u, v, level, desc, gate, z=1.0, max_d=None, min_d=None, bad=0, skip=0, xyz=None):
        x, y, z = xyz if xyz is not None else back_project(u, v, z)
        dist = norm3(x, y, z)
        max_d = max_distance_for(dist, level) if max_d is None else max_d(dist) if callable(max_d) else f32(max_d)
        min_d = f32(max_d / f32(4.0)) if min_d is None else min_d(dist) if callable(min_d) else f32(min_d)
        pts.append((x, y, z, min_d, max_d, bad, 1, skip))
        mpd.append(desc)
        cases.append((len(pts) - 1, gate))
        while pending:   # the keypoints planted since the last point were planted for this one
            owner[pending.pop()] = len(pts) - 1
        return len(pts) - 1

    owner, pending = {}, []

    def kpt(x, y, octave, desc, ur=-1.0, taken=0):
        pending.append(F.add(x, y, octave, desc, u_right=f32(ur), taken=taken))
        return pending[-1]

    # --- Hamming ties ---
    u, v, P = new_site()
    kpt(u + 2, v + 2, 1, flip(P, 0, 20)); kpt(u + 6, v + 6, 2, flip(P, 40, 20))
    point(u + 4, v + 4, 2, P, "tie between cells (k, m) and (k + 1, m + 1), levels lvl - 1 and lvl: the first visited wins")
    u, v, P = new_site()
    kpt(u + 1, v, 2, flip(P, 0, 20)); kpt(u + 1.5, v, 2, flip(P, 40, 20)); kpt(u + 0.5, v, 2, flip(P, 80, 21))
    point(u, v, 2, P, "tie inside one cell: the lower index wins")
    u, v, P = new_site()
    kpt(u + 3, v + 5, 2, flip(P, 0, 20)); kpt(u + 5, v + 3, 2, flip(P, 40, 20))
    point(u + 4, v + 4, 2, P, "tie between cells (x0, y1) and (x1, y0): columns are walked before rows")
    u, v, P = new_site()
    kpt(u + 4.8 - 4, v, 2, flip(P, 0, 20)); kpt(u + 1.6 - 4, v, 2, flip(P, 40, 20))
    point(u - 3, v, 2, P, "tie between a keypoint at 0.6 of a cell and a later one in the cell below")
    # --- window: |dx| < r with r = 3 at level 0 (stereo-free keypoints; chi-square passes only near the centre, so the
    #     Sim3 overload, which has no chi-square gate, is the one that sees these) ---
    for axis in "xy":
        for sign in (1, -1):
            for which in (0, 1):
                u, v, P = new_site()
                pos = offset_exact(u if axis == "x" else v, f32(FUSE_TH), sign)[which]
                kpt(pos if axis == "x" else u, pos if axis == "y" else v, 0, flip(P, 0, 10))
                point(u, v, 0, P, "keypoint %s r in %s%s" % (("exactly at", "one unit inside")[which], "+-"[sign < 0], axis), max_d=lambda d: f32(d * f32(0.95)))
    # --- level pair ---
    for lvl, octv, gate in ((3, 1, "only lvl - 2: refused"), (3, 2, "only lvl - 1"), (3, 3, "only lvl"), (3, 4, "only lvl + 1: refused (the relocalisation search takes it)"), (3, 5, "only lvl + 2: refused"),
                            (0, 0, "level 0, octave 0"), (0, 1, "level 0, octave 1: refused"), (7, 6, "q in (7, 8): ceil gives 8, clamped to 7; octave 6")):
        u, v, P = new_site()
        kpt(u + 1, v, octv, flip(P, 0, 10))
        point(u, v, lvl, P, gate, max_d=(lambda d: f32(np.float64(d) * 1.2 ** 7.5)) if lvl == 7 else None)
    # --- predicted level exactly on an integer and one unit either side ---
    for kk in (1, 2, 3, 5):
        u, v, P = new_site()
        x, y, z = back_project(u, v)
        below, exact, above = level_edge(norm3(x, y, z), kk)
        kpt(u + 1, v, kk - 1, flip(P, 0, 10)); kpt(u - 1, v, kk + 1, flip(P, 40, 9))   # lvl == kk sees the first, lvl == kk + 1 the second
        point(u, v, kk, P, "q one unit below %d" % kk, max_d=below)
        point(u, v, kk + 1, P, "q one unit above %d: level %d" % (kk, kk + 1), max_d=above)
        for m in exact[:2]:
            point(u, v, kk, P, "q exactly %d: level %d" % (kk, kk), max_d=m)
    # --- thresholds and taken keypoints of the searches that have them (SearchBySim3, relocalisation); Fuse returns them as they are ---
    for dd, gate in ((TH_HIGH, "best == TH_HIGH"), (TH_HIGH + 1, "best == TH_HIGH + 1")):
        u, v, P = new_site(); kpt(u + 1, v, 1, flip(P, 0, dd))
        point(u, v, 1, P, gate)
    u, v, P = new_site(); kpt(u + 1, v, 1, flip(P, 0, 5), taken=1); kpt(u - 1, v, 1, flip(P, 40, 50))
    point(u, v, 1, P, "the nearer keypoint already holds a map point (relocalisation)")
    # --- distance gates ---
    u, v, P = new_site(); kpt(u + 1, v, 0, flip(P, 0, 10))
    point(u, v, 0, P, "dist3D == 0.9f * minDistance exactly: kept", max_d=lambda d: f32(d * f32(1.05)), min_d=lambda d: scaled_bound(d, 0.9))
    point(u, v, 0, P, "dist3D one unit below 0.9f * minDistance: dropped", max_d=lambda d: f32(d * f32(1.05)), min_d=lambda d: nxt(scaled_bound(d, 0.9), 2))
    u, v, P = new_site(); kpt(u + 1, v, 0, flip(P, 0, 10))
    point(u, v, 0, P, "dist3D == 1.1f * maxDistance exactly: kept", max_d=lambda d: scaled_bound(d, 1.1), min_d=0.1)
    point(u, v, 0, P, "dist3D one unit above 1.1f * maxDistance: dropped", max_d=lambda d: nxt(scaled_bound(d, 1.1), -2), min_d=0.1)
    u, v, P = new_site(); kpt(u, v, 0, flip(P, 0, 10))
    x, y, z, d = split_bound(u, v, 0.9, 0.9, True)
    point(u, v, 0, P, "dist3D == 0.9f * minDistance, but below (float)(0.9 * minDistance): kept", xyz=(x, y, z), max_d=lambda dd: f32(dd * f32(1.05)), min_d=d)
    u, v, P = new_site(); kpt(u, v, 0, flip(P, 0, 10))
    x, y, z, d = split_bound(u, v, 1.1, 1.1, False)
    point(u, v, 0, P, "dist3D == 1.1f * maxDistance, but above (float)(1.1 * maxDistance): kept", xyz=(x, y, z), max_d=d, min_d=0.1)
    u, v, P = new_site(); kpt(u + 1, v, 0, flip(P, 0, 10))
    point(u, v, 0, P, "far beyond maxDistance", max_d=lambda d: f32(d * f32(0.5)), min_d=0.1)
    point(u, v, 0, P, "far below minDistance", max_d=lambda d: f32(d * f32(8)), min_d=lambda d: f32(d * f32(2)))
    # --- point gates ---
    u, v, P = new_site(); kpt(u + 1, v, 1, flip(P, 0, 10))
    point(u, v, 1, P, "bad", bad=1)
    u, v, P = new_site(); kpt(u + 1, v, 1, flip(P, 0, 10))
    point(u, v, 1, P, "skip", skip=1)
    u, v, P = new_site(); kpt(u + 1, v, 1, flip(P, 0, 10))
    x, y, z = back_project(u, v)
    point(u, v, 1, P, "behind the camera: (-x, -y, -1) would project onto the same keypoint", xyz=(f32(-x), f32(-y), f32(-1.0)))
    point(u, v, 1, P, "depth 0, off the axis: the projection is infinite", xyz=(x, y, f32(0.0)), max_d=4.0, min_d=0.01)
    # --- image bounds (KeyFrame::IsInImage is half open).  A keypoint within 4 pixels of maxX or maxY rounds to column 64 / row 48,
    #     which PosInGrid files under the next row / refuses: the cases at those two bounds use level 5 (r = 7.46) and a keypoint 4.5 away ---
    P = pattern(70)
    xl, xr, yt, yb = f32((MINX - CX) / FX), f32((MAXX - CX) / FX), f32((MINY - CY) / FY), f32((MAXY - CY) / FY)
    for x, y, kx, ky, lvl, gate in ((xl, None, MINX + 1, None, 0, "u == minX: inside"), (nxt(xl, -1), None, MINX + 1, None, 0, "u just below minX: outside"),
                                    (xr, None, MAXX - 4.5, None, 5, "u == maxX: outside"), (nxt(xr, -1), None, MAXX - 4.5, None, 5, "x one unit below, u rounds to maxX: outside"),
                                    (nxt(xr, -3), None, MAXX - 4.5, None, 5, "u one unit below maxX: inside"),
                                    (None, yt, None, MINY + 1, 0, "v == minY: inside"), (None, nxt(yt, -1), None, MINY + 1, 0, "v just below minY: outside"),
                                    (None, yb, None, MAXY - 4.5, 5, "v == maxY: outside"), (None, nxt(yb, -1), None, MAXY - 4.5, 5, "v one unit below maxY: inside")):
        u, v, _ = new_site()   # the free coordinate comes from a lattice site
        x, y = (f32((u - CX) / FX) if x is None else x), (f32((v - CY) / FY) if y is None else y)
        up, vp = f32(f32(f32(FX) * x) + f32(CX)), f32(f32(f32(FY) * y) + f32(CY))
        kpt(u if kx is None else kx, v if ky is None else ky, lvl, flip(P, 0, 10))
        point(up, vp, lvl, P, gate, xyz=(x, y, f32(1.0)), max_d=(lambda d: f32(d * f32(0.95))) if lvl == 0 else None)
    # --- chi-square gates ---
    u, v, P = new_site()
    unit = float(max(np.spacing(f32(u)), np.spacing(f32(v))))
    ex, ey, _ = chi2_values(unit, INV_S2[0], f32(5.99), 2)
    kpt(f32(u - ex), f32(v - ey), 0, flip(P, 0, 10))
    assert f32(f32(f32(u - f32(u - ex)) ** 2 + f32(v - f32(v - ey)) ** 2) * INV_S2[0]) == f32(5.99)
    point(u, v, 0, P, "mono chi-square == 5.99f exactly (below the double 5.99): kept", max_d=lambda d: f32(d * f32(0.95)))
    u, v, P = new_site()
    kpt(f32(u - nxt(ex, 40)), f32(v - ey), 0, flip(P, 0, 10))
    point(u, v, 0, P, "mono chi-square just above 5.99: dropped", max_d=lambda d: f32(d * f32(0.95)))
    u, v, P = new_site()
    unit = float(max(np.spacing(f32(u)), np.spacing(f32(v))))
    ex3, ey3, er3 = chi2_values(unit, INV_S2[0], f32(7.8), 3)
    assert f32(f32(f32(f32(u - f32(u - ex3)) ** 2 + f32(v - f32(v - ey3)) ** 2) + er3 * er3) * INV_S2[0]) == f32(7.8)
    kpt(f32(u - ex3), f32(v - ey3), 0, flip(P, 0, 10), ur=f32(f32(u - f32(MBF)) - er3))
    point(u, v, 0, P, "stereo chi-square == 7.8f exactly (above the double 7.8): dropped; the mono value passes", max_d=lambda d: f32(d * f32(0.95)))
    u, v, P = new_site()
    kpt(f32(u - nxt(ex3, -40)), f32(v - ey3), 0, flip(P, 0, 10), ur=f32(f32(u - f32(MBF)) - er3))
    point(u, v, 0, P, "stereo chi-square just below 7.8: kept", max_d=lambda d: f32(d * f32(0.95)))
    u, v, P = new_site()
    kpt(u + 1, v, 0, flip(P, 0, 10), ur=0.0)
    point(u, v, 0, P, "uRight == 0 exactly: a stereo keypoint, whose right error is huge", max_d=lambda d: f32(d * f32(0.95)))
    u, v, P = new_site()
    kpt(u + 2, v + 2, 0, flip(P, 0, 10)); kpt(u + 0.5, v, 0, flip(P, 40, 50)); kpt(u + 1, v + 1, 0, flip(P, 90, 11), ur=f32(u + 1 - MBF - 3))
    point(u, v, 0, P, "the nearer descriptors fail the mono (8 > 5.99) and the stereo (11 > 7.8) gate", max_d=lambda d: f32(d * f32(0.95)))
    u, v, P = new_site()   # level 3, keypoint on level 2: e2 = 13 -> 13 / 2.0736 = 6.27 > 5.99 with its own sigma, 13 / 2.986 = 4.35 with lvl's
    kpt(u + 3, v + 2, 2, flip(P, 0, 10)); kpt(u, v + 1, 3, flip(P, 40, 50))
    point(u, v, 3, P, "the gate reads the sigma of the keypoint's level, not of the predicted one (mono)")
    u, v, P = new_site()   # stereo: e2 = 9 + 4 + 4 = 17 -> 8.2 > 7.8 on level 2, 5.7 on level 3
    kpt(u + 3, v + 2, 2, flip(P, 0, 10), ur=f32(u - MBF - 2)); kpt(u, v + 1, 3, flip(P, 40, 50), ur=f32(u - MBF))
    point(u, v, 3, P, "the same for the stereo gate")
    # --- candidate-sink crowd: 16, 17 and 24 keypoints pass every gate of one point; the best comes late in the visit order ---
    for count in (16, 17, 24):
        u, v, P = new_site()
        mine = []
        for j in range(count):   # a 5 x 5 raster of 0.4-pixel steps around (u + 4, v + 4): four cells, level 2
            best = j == max(i for i in range(count) if i % 5 >= 2 and i // 5 >= 2)   # the last one visited: last cell, highest index
            mine.append(kpt(u + 4 + 0.4 * (j % 5 - 2) + 0.1, v + 4 + 0.4 * (j // 5 - 2) + 0.1, 2, flip(P, 3 * j, 9 if best else 12 + j % 7)))
        crowd.append((point(u + 4, v + 4, 2, P, "%d keypoints pass every gate" % count), mine))
    # the row limit of the right-camera call: the last planted keypoint is the first one without a right twin
    u, v, P = new_site()
    kpt(u + 1, v, 0, flip(P, 0, 12)); last = kpt(u - 1, v, 0, flip(P, 40, 10))
    row_limit = point(u, v, 0, P, "bRight: idx == nRight has no right row", max_d=lambda d: f32(d * f32(0.95)))
    for j in range(10):   # plain pairs: the ones a rotation plan may put into the losing bins
        u, v, P = new_site(); kpt(u + 1, v + 1, 1, flip(P, 0, 8 + j))
        point(u, v, 1, P, "plain pair %d" % j)
    assert k[0] <= 84, k[0]

    for j in range(pad_points):
        x, y, z = back_project(*inert_spot(j))
        d = norm3(x, y, z)
        pts.append((x, y, z, f32(0.1), f32(d * f32(0.95)), 0, 1, int(j % 5 == 0)))   # level 0
        mpd.append(pattern(100 + j))
    kp, desc, extras, first = F.build(pad, defaults=dict(u_right=f32(-1.0), taken=0))
    n, n_right = len(kp), first(last)
    crowd = [(i, [first(j) for j in mine]) for i, mine in crowd]   # (point, its keypoints: every one passes every gate of that point)
    # mDescriptors of a two-camera key frame: the left rows, then the right twins (a few other bits flipped), then ONE spare row
    # beyond the matrix that holds the row-limit point's own descriptor -- no call may read it
    store = np.zeros((n + n_right + 1, 32), np.uint8)
    store[:n] = desc
    for i in range(n_right):
        store[n + i] = flip(desc[i], 128 + i % 64, i % 5)
    store[n + n_right] = mpd[row_limit]
    return dict(kp=kp, desc=desc, desc_lr=store[:n + n_right], n_right=n_right, u_right=extras["u_right"].astype(np.float32),
                taken=extras["taken"].astype(np.uint8), owner={first(j): i for j, i in owner.items()},
                pts=np.array(pts, dtype=O.WP_DTYPE), mpDesc=np.ascontiguousarray(np.stack(mpd)), cases=cases, crowd=crowd, pad=pad)


def fuse_scenes(pad=0, pad_points=0):
    w = fuse_world(pad, pad_points)
    size = "bare" if not pad else "padded-%d" % len(w["kp"])
    common = dict(kp=w["kp"], invLevelSigma2=INV_S2, frustum=FRUSTUM, th=FUSE_TH, pts=w["pts"], mpDesc=w["mpDesc"])
    mk = lambda matcher, name, **a: dict(matcher=matcher, name=name, size=size, cases=w["cases"], crowd=w["crowd"], args=dict(common, **a))
    return [mk("fuse", "fuse-mono", desc=w["desc"], uRight=None), mk("fuse", "fuse-stereo", desc=w["desc"], uRight=w["u_right"]),
            mk("fuse_right", "fuse-right", desc=w["desc_lr"], uRight=w["u_right"], nRight=w["n_right"]),
            mk("fuse_sim3", "fuse-sim3", desc=w["desc"]), reloc_scene(w, size), sim3_scene(w, size)]


def reloc_scene(w, size):
    """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, checkOrientation) on the Fuse cases: the frame is the
    Fuse key frame, the key frame's map points are the Fuse points.  Three levels (lvl - 1 .. lvl + 1), closed image bounds, no depth
    test, taken keypoints, TH_HIGH, and the rotation histogram with the "edges" plan on the pairs that exist without it."""
    a = dict(kp=w["kp"].copy(), desc=w["desc"], frustum=FRUSTUM, pts=w["pts"], mpDesc=w["mpDesc"], kfAngle=np.zeros(len(w["pts"]), np.float32),
             frameHasMP=w["taken"], th=FUSE_TH, checkOrientation=True)
    a["kp"]["angle"] = 0.0
    _, m = O.search_by_projection_kf(view(a["kp"], a["desc"]), frustum(O.Frustum, ORACLE_NAMES), a["pts"], a["mpDesc"], a["kfAngle"], a["frameHasMP"], a["th"], False)
    plain = {i for i, g in w["cases"] if g.startswith("plain pair")}
    pairs = sorted(np.flatnonzero(m >= 0), key=lambda i2: (m[i2] in plain, i2))   # the plain pairs last: they take the losing bins
    for i2, (a1, a2) in zip(pairs, rotation_angles("edges", len(pairs))):
        a["kfAngle"][m[i2]], a["kp"]["angle"][i2] = a1, a2
    return dict(matcher="projection_kf", name="relocalisation", size=size, cases=w["cases"], args=a)


def sim3_dir(cls):
    D = cls()
    vals = [(1, 0, 0, 0, 1, 0, 0, 0, 1), (0, 0, 0), (1, 0, 0, 0, 1, 0, 0, 0, 1), (0, 0, 0), FX, FY, CX, CY, MINX, MAXX, MINY, MAXY, float(LOG_SF), NLEVELS]
    for (name, _), v in zip(cls._fields_, vals):
        if isinstance(v, tuple):
            for i, y in enumerate(v):
                getattr(D, name)[i] = float(y)
        else:
            setattr(D, name, v)
    return D


def sim3_scene(w, size):
    """ORBmatcher::SearchBySim3 with identity poses and similarity.  Key frame 2 is the Fuse key frame and key frame 1's map points
    are the Fuse points, so direction 1 -> 2 walks the Fuse cases (half-open bounds, depth sign, levels lvl - 1 / lvl, TH_HIGH, no
    chi-square).  Key frame 1 has one keypoint per point, at the point's projection, carrying the point's descriptor; the map point of
    a planted keypoint of key frame 2 sits on the key-frame-1 keypoint of the point it was planted for, with that point's descriptor,
    so direction 2 -> 1 answers with that point and the agreement loop passes what direction 1 -> 2 found for it."""
    pts, n2 = w["pts"], len(w["kp"])
    kp1 = np.zeros(len(pts), O.KP_DTYPE)
    for i, p in enumerate(pts):
        z = p["z"] if p["z"] > 0 else f32(1.0)
        u, v = f32(f32(FX) * f32(p["x"] / z) + f32(CX)), f32(f32(FY) * f32(p["y"] / z) + f32(CY))
        if not (MINX <= u < MAXX - 4 and MINY <= v < MAXY - 4) or p["z"] <= 0:   # no projection to sit on: a raster below the sites
            u, v = f32(MINX + 6 + 6 * (i % 80)), f32(MINY + 300 + 6 * (i // 80 % 14))
        kp1[i] = (u, v, 50, 31.0, predict_level(p["maxDistance"], norm3(p["x"], p["y"], p["z"])), 0.0)
    mp2 = np.zeros(n2, O.WP_DTYPE)
    mp2["skip"] = 1                                  # filler keypoints have no map point
    desc_mp2 = w["desc"].copy()
    for j, i in w["owner"].items():                   # the map point of a planted keypoint of key frame 2 sits on the keypoint of key frame 1
        x, y = f32((kp1[i]["x"] - f32(CX)) / f32(FX)), f32((kp1[i]["y"] - f32(CY)) / f32(FY))   # that belongs to the point it was planted for
        d = norm3(x, y, f32(1))
        mp2[j] = (x, y, 1.0, 0.05, f32(np.float64(d) * 1.2 ** (int(kp1[i]["octave"]) - 0.5)), 0, 1, 0)
        desc_mp2[j] = w["mpDesc"][i]
    return dict(matcher="sim3", name="sim3", size=size, cases=w["cases"],
                args=dict(kp1=kp1, desc1=w["mpDesc"], kp2=w["kp"], desc2=w["desc"], mp1=pts, mpDesc1=w["mpDesc"], mp2=mp2, mpDesc2=desc_mp2, th=FUSE_TH))


def oracle_projection_kf(a):
    n, m = O.search_by_projection_kf(view(a["kp"], a["desc"]), frustum(O.Frustum, ORACLE_NAMES, a["frustum"]), a["pts"], a["mpDesc"], a["kfAngle"],
                                     a["frameHasMP"], a["th"], a["checkOrientation"])
    return dict(n=np.int64(n), match=m)


def oracle_sim3(a):
    n, m = O.search_by_sim3(view(a["kp1"], a["desc1"]), view(a["kp2"], a["desc2"]), sim3_dir(O.Sim3Dir), sim3_dir(O.Sim3Dir), a["mp1"], a["mpDesc1"],
                            a["mp2"], a["mpDesc2"], a["th"])
    return dict(n=np.int64(n), match=m)


def oracle_fuse(a):
    bi, bd = O.fuse_search(view(a["kp"], a["desc"]), a["invLevelSigma2"], a["uRight"], frustum(O.Frustum, ORACLE_NAMES, a["frustum"]), a["th"],
                           a["pts"], a["mpDesc"])
    return dict(bestIdx=bi, bestDist=bd)


def oracle_fuse_right(a):
    bi, bd = O.fuse_search_right(view(a["kp"], a["desc"]), a["nRight"], a["invLevelSigma2"], a["uRight"],
                                 frustum(O.Frustum, ORACLE_NAMES, a["frustum"]), a["th"], a["pts"], a["mpDesc"])
    return dict(bestIdx=bi, bestDist=bd)


def oracle_fuse_sim3(a):
    bi, bd = O.fuse_search_sim3(view(a["kp"], a["desc"]), frustum(O.Frustum, ORACLE_NAMES, a["frustum"]), a["th"], a["pts"], a["mpDesc"])
    return dict(bestIdx=bi, bestDist=bd)


def visit_order(kp, desc, idx):
    """the keypoints `idx` in the order GetFeaturesInArea visits them: cell column, cell row, index"""
    cell = O.assign_grid(view(kp, desc))
    return sorted(idx, key=lambda i: (cell[i] % COLS, cell[i] // COLS, i))


# ======================================================================================================================
# Frame::isInFrustum: points only.  Its image test is closed on both sides (u == maxX is inside), unlike KeyFrame::IsInImage.
# ======================================================================================================================
def frustum_scene(pad_points=0):
    pts, cases = [], []

    def point(gate, x, y, z=1.0, level=2, max_d=None, min_d=None, bad=0, skip=0):
        x, y, z = f32(x), f32(y), f32(z)
        dist = norm3(x, y, z)
        max_d = max_distance_for(dist, level) if max_d is None else max_d(dist) if callable(max_d) else f32(max_d)
        min_d = f32(max_d / f32(4.0)) if min_d is None else min_d(dist) if callable(min_d) else f32(min_d)
        pts.append((x, y, z, min_d, max_d, bad, 1 + len(pts) % 3, skip))
        cases.append((len(pts) - 1, gate))

    xl, xr, yt, yb = f32((MINX - CX) / FX), f32((MAXX - CX) / FX), f32((MINY - CY) / FY), f32((MAXY - CY) / FY)
    point("plain", 0.25, 0.125)
    point("bad", 0.25, 0.125, bad=1); point("skip", 0.25, 0.125, skip=1)
    point("behind the camera", 0.25, 0.125, z=-1.0); point("depth 0 off the axis: infinite projection", 0.25, 0.125, z=0.0, max_d=4.0, min_d=0.01)
    for x, gate in ((xl, "u == minX: inside"), (nxt(xl, -1), "u just below minX"), (xr, "u == maxX: inside (closed bound)"),
                    (nxt(xr, 1), "x one unit above, u rounds to maxX: inside"), (nxt(xr, 3), "u just above maxX")):
        point(gate, x, 0.125)
    for y, gate in ((yt, "v == minY: inside"), (nxt(yt, -1), "v just below minY"), (yb, "v == maxY: inside (closed bound)"),
                    (nxt(yb, 1), "y one unit above, v rounds to maxY: inside"), (nxt(yb, 3), "v just above maxY")):
        point(gate, 0.25, y)
    d = norm3(f32(0.5), f32(0.25), f32(1))
    point("dist == 0.9f * minDistance exactly", 0.5, 0.25, max_d=lambda d: f32(d * f32(1.5)), min_d=lambda d: scaled_bound(d, 0.9))
    point("dist one unit below 0.9f * minDistance: projection written, not in view", 0.5, 0.25, max_d=lambda d: f32(d * f32(1.5)), min_d=lambda d: nxt(scaled_bound(d, 0.9), 2))
    point("dist == 1.1f * maxDistance exactly", 0.5, 0.25, max_d=lambda d: scaled_bound(d, 1.1), min_d=0.1)
    point("dist one unit above 1.1f * maxDistance", 0.5, 0.25, max_d=lambda d: nxt(scaled_bound(d, 1.1), -2), min_d=0.1)
    x, y, z, m = split_bound(CX + 100, CY + 50, 0.9, 0.9, True)
    point("dist == 0.9f * minDistance but below (float)(0.9 * minDistance)", x, y, z, max_d=lambda d: f32(d * f32(1.5)), min_d=m)
    x, y, z, m = split_bound(CX + 100, CY + 50, 1.1, 1.1, False)
    point("dist == 1.1f * maxDistance but above (float)(1.1 * maxDistance)", x, y, z, max_d=m, min_d=0.1)
    for kk in range(1, NLEVELS + 1):
        below, exact, above = level_edge(d, kk)
        point("q one unit below %d" % kk, 0.5, 0.25, max_d=below, min_d=0.1); point("q one unit above %d" % kk, 0.5, 0.25, max_d=above, min_d=0.1)
        for m in exact[:2]:
            point("q exactly %d" % kk, 0.5, 0.25, max_d=m, min_d=0.1)
    point("ratio 1: q == 0", 0.5, 0.25, max_d=d, min_d=0.1); point("ratio below 1: q < 0", 0.5, 0.25, max_d=lambda d: f32(d * f32(0.95)), min_d=0.1)
    point("q far above nLevels", 0.5, 0.25, max_d=lambda d: f32(d * f32(30)), min_d=0.1)
    for j in range(pad_points):
        point("filler", -0.9 + 1.8 * (j % 97) / 97.0, -0.7 + 1.4 * (j % 89) / 89.0, z=1.0 + (j % 5) * 0.5, level=j % NLEVELS, bad=int(j % 31 == 0), skip=int(j % 29 == 0))
    return dict(matcher="frustum", name="frustum", size="bare" if not pad_points else "padded-%d" % len(pts), cases=cases[:len(cases) - pad_points],
                args=dict(frustum=FRUSTUM, pts=np.array(pts, dtype=O.WP_DTYPE)))


def oracle_frustum(a):
    out, xr = O.is_in_frustum(frustum(O.Frustum, ORACLE_NAMES, a["frustum"]), a["pts"])
    return dict(records=out, projXR=xr)


# ======================================================================================================================
# Rotation histogram: the matchers put rot = angle1 - angle2 (+ 360 if negative) into bin round(rot / 30) and keep the three fullest
# bins.  A plan gives the matched pairs (those whose feature has exactly one match) their rotation differences.
# ======================================================================================================================
ROT = {0: (0.0, 0.0), 2: (60.0, 0.0), 5: (150.0, 0.0), 9: (0.0, 90.0), 10: (289.0, 0.0), 12: (355.0, 0.0), 30: (899.0, 0.0)}
# bin -> (angle of the first feature, angle of the second): bin 9 through a negative difference, bin 10 only by rounding (9.63),
# bin 12 = 11.83 rounded, 30 = a difference of 899 degrees (round(29.97) == 30 -> bin 0; no extractor gives such an angle, no
# contract forbids it)


SPARE_BINS = (1, 3, 4, 6, 7, 8, 11)


def rotation_plan(plan, n):
    """bins of n matched pairs; what a plan does not need goes one or two at a time into bins that stay below third place"""
    spare = lambda k: [SPARE_BINS[j % 7] for j in range(k)]
    if plan == "edges":     # bin 0: an exact zero and an 899, twice (SearchByBoW: once per camera); bin 2: up to 29; bin 5: 5 and more;
        keep = [0, 30, 0, 30] + [5] * 5   # then the losers 9: 4, 12: 4, 10: 1 -- third place is a tie 0 / 9 / 12, which the earliest bin wins
        lose = [9] * 4 + [12] * 4 + [10]
        rest = n - len(keep) - len(lose)
        assert rest >= 6
        more5 = max(0, min(rest - 29, 23))   # bin 5 stays below bin 2
        return keep + [2] * min(rest, 29) + [5] * more5 + lose + spare(rest - min(rest, 29) - more5)
    if plan == "ties":      # four bins equally full: first, second and third place are all ties
        q = n // 4
        assert q >= 2
        return [2] * q + [5] * q + [9] * q + [12] * q + spare(n - 4 * q)
    if plan == "tenth2":    # max2 == max3 == max1 / 10 exactly: (float)max2 < 0.1f * (float)max1 is false at equality
        m = n // 12
        assert m >= 3
        return [2] * (10 * m) + [5] * m + [9] * m + spare(n - 12 * m)
    assert plan == "tenth3"  # max3 == max1 / 10, max2 above
    m = n // 16
    extra = max(0, n - 16 * m - 7)    # what the spare bins cannot take singly makes second place fuller
    assert m >= 2 and extra < 5 * m
    return [2] * (10 * m) + [5] * (5 * m + extra) + [9] * m + spare(n - 16 * m - extra)


def rotation_angles(plan, n):
    out = []
    for b in rotation_plan(plan, n):
        out.append(ROT[b] if b in ROT else (30.0 * b, 0.0))
    return out


# ======================================================================================================================
# ORBmatcher::SearchByBoW: nodes of (key-frame features, frame features); no geometry
# ======================================================================================================================
def bow_world(rig, node_size=0, kf_node_size=0):
    nodes, cases = [], []

    def node(kfs, fs, gate):
        """kfs: [(desc, hasMP)], fs: [(desc, side)]"""
        nodes.append((kfs, fs))
        cases.append((len(nodes) - 1, gate))

    g = [0]

    def P():
        g[0] += 1
        return pattern(g[0] - 1)

    p = P(); f0 = flip(p, 0, 5); kb = flip(f0, 100, 3)
    node([(p, 1), (kb, 1)], [(f0, "L"), (flip(kb, 150, 25), "L")], "key-frame feature 0 matches; a later, nearer one must skip the matched frame feature")
    p = P()
    node([(p, 1)], [(flip(p, 0, 25), "L"), (flip(p, 40, 5), "R")], "the frame feature with index == nLeft belongs to the right camera")
    p = P(); node([(p, 0)], [(flip(p, 0, 5), "L")], "key-frame feature without a map point")
    p = P(); node([(p, 1)], [(flip(p, 0, TH_LOW), "L")], "best == TH_LOW: matched")
    p = P(); node([(p, 1)], [(flip(p, 0, TH_LOW + 1), "L")], "best == TH_LOW + 1: refused")
    p = P(); node([(p, 1)], [(flip(p, 0, 40), "L"), (flip(p, 60, 30), "L")], "ratio at float equality 30 == 0.75 * 40: refused (strict <)")
    p = P(); node([(p, 1)], [(flip(p, 0, 40), "L"), (flip(p, 60, 29), "L")], "ratio passed")
    p = P(); node([(p, 1)], [(flip(p, 0, 20), "L"), (flip(p, 40, 40), "L"), (flip(p, 90, 40), "L")], "tie in second best")
    p = P(); node([(p, 1)], [(flip(p, 0, 20), "L"), (flip(p, 40, 20), "L")], "tie in best: refused by any ratio below 1, the first wins at ratio 1.5")
    p = P(); node([(p, 1)], [(flip(p, 0, 10), "L"), (flip(p, 40, 12), "R")], "left and right match")
    p = P(); node([(p, 1)], [(flip(p, 0, 10), "L"), (flip(p, 40, 15), "R"), (flip(p, 80, 15), "R")], "tie in the right camera's best (no ratio test there): the first wins")
    p = P(); node([(p, 1)], [(flip(p, 0, 10), "L"), (flip(p, 40, TH_LOW), "R")], "right best == TH_LOW: matched")
    p = P(); node([(p, 1)], [(flip(p, 0, 10), "L"), (flip(p, 40, TH_LOW + 1), "R")], "right best == TH_LOW + 1: refused")
    p = P(); node([(p, 1)], [(flip(p, 0, TH_LOW + 1), "L"), (flip(p, 40, 10), "R")], "left best above TH_LOW: the right match is not even tried")
    for j in range(4):   # the only way to a right pair alone: the right side is tried when the left best passes TH_LOW, whatever its ratio says
        p = P(); node([(p, 1)], [(flip(p, 0, 30), "L"), (flip(p, 40, 31), "L"), (flip(p, 80, 10 + j), "R")], "left fails its ratio, right matches (%d)" % j)
    p = P(); node([(p, 1)], [(flip(p, 0, 12), "R"), (flip(p, 40, 10), "L")], "right feature earlier in the node's list than the left one")
    for j in range(34):
        p = P(); node([(p, 1)], [(flip(p, 0, 8 + j % 5), "L")], "plain pair %d (rotation histogram)" % j)

    far = lambda j: np.roll(Frame.filler(j)["desc"], j % 7)   # inert key-frame features: >= 140 bits from every planted frame feature

    def low(j):   # inert frame features: at most 5 ones, so >= 59 bits from every planted key-frame pattern (64 ones), ~250 from far()
        d = np.zeros(32, np.uint8)
        d[j % 32] = j % 251 & 0x1F
        return d
    kf_desc, kf_has, kf_of = [], [], []
    side_desc = {"L": [], "R": []}
    f_of = {"L": [], "R": []}          # per side: (node, position key) in list order
    for gi, (kfs, fs) in enumerate(nodes):
        kpad = max(0, kf_node_size - len(kfs))
        klist = [(far(1000 + gi * 7 + j), 1) for j in range(kpad // 2)] + kfs + [(far(2000 + gi * 7 + j), 1) for j in range(kpad - kpad // 2)]
        if gi == 0:
            klist = kfs + [(far(1000 + j), 1) for j in range(kpad)]   # key-frame feature 0 stays feature 0
        for d, h in klist:
            kf_desc.append(d); kf_has.append(h); kf_of.append(gi)
        fpad = max(0, node_size - len(fs))
        sd_of = lambda j: "LR"[j % 2] if rig and gi > 0 else "L"   # node 0 is padded on the left only: node 1 plants the FIRST right feature
        flist = [(low(3000 + gi * 11 + j), sd_of(j)) for j in range(fpad // 2)] + fs + [(low(4000 + gi * 11 + j), sd_of(j)) for j in range(fpad - fpad // 2)]
        if gi == 1:
            flist = fs + [(low(3000 + j), sd_of(j)) for j in range(fpad)]   # its right feature stays the first right one
        for pos, (d, sd) in enumerate(flist):
            side_desc[sd].append(d); f_of[sd].append((gi, pos))
    n_left = len(side_desc["L"])
    f_desc = np.ascontiguousarray(np.stack(side_desc["L"] + side_desc["R"]))
    # CSR in node order; inside a node the frame features in the node's list order (left and right interleaved as planted)
    entries = [(gi, pos, i) for i, (gi, pos) in enumerate(f_of["L"] + f_of["R"])]
    entries.sort()
    fIdx = [i for _, _, i in entries]
    fOff = [0] + list(np.cumsum(np.bincount([gi for gi, _, _ in entries], minlength=len(nodes))))
    kfIdx = list(range(len(kf_desc)))
    kfOff = [0] + list(np.cumsum(np.bincount(kf_of, minlength=len(nodes))))
    return dict(kfOff=np.array(kfOff, np.int32), kfIdx=np.array(kfIdx, np.int32), fOff=np.array(fOff, np.int32), fIdx=np.array(fIdx, np.int32),
                kfDesc=np.ascontiguousarray(np.stack(kf_desc)), kfHasMP=np.array(kf_has, np.uint8), fDesc=f_desc,
                nLeft=n_left if rig else -1, cases=cases)


def bow_scene(plan, rig, nn=0.75, node_size=0, kf_node_size=0):
    w = bow_world(rig, node_size, kf_node_size)
    cases = w.pop("cases")
    a = dict(w, nnRatio=nn, checkOrientation=plan is not None, kfAngle=np.zeros(len(w["kfDesc"]), np.float32), fAngle=np.zeros(len(w["fDesc"]), np.float32))
    if plan is not None:   # which pairs exist does not depend on the angles: the histogram only deletes
        _, m = O.search_by_bow(a["kfOff"], a["kfIdx"], a["fOff"], a["fIdx"], a["kfDesc"], a["kfAngle"], a["kfHasMP"], a["fDesc"], a["fAngle"], nn, False, nLeft=a["nLeft"])
        count = np.bincount(m[m >= 0], minlength=len(a["kfDesc"]))
        single = [int(i) for i in np.flatnonzero(m >= 0) if count[m[i]] == 1]
        bins = rotation_plan(plan, len(single))
        right = [f for f in single if a["nLeft"] >= 0 and f >= a["nLeft"]]
        if right:   # the right camera has its own copy of the histogram lines: two of its pairs take the third and fourth entry of the plan
            assert len(right) >= 3 and 9 in bins   # (edges: the second exact zero and the second 899), one the first negative difference (bin 9)
            spots = [2, 3, bins.index(9)]
            left = [f for f in single if f not in right[:3]]
            single = left
            for spot, f in sorted(zip(spots, right[:3])):
                single.insert(spot, f)
        for f, (a1, a2) in zip(single, rotation_angles(plan, len(single))):
            a["kfAngle"][m[f]], a["fAngle"][f] = a1, a2
        twice = np.flatnonzero(count > 1)
        a["kfAngle"][twice] = 60.0   # a key-frame feature matched in both cameras: both pairs in bin 2 ...
        if plan == "edges" and len(twice):
            a["kfAngle"][twice[0]] = 289.0   # ... but for one, whose two pairs fall into bin 10 by rounding only
    size = "bare" if not (node_size or kf_node_size) else "padded-node%d-kf%d" % (node_size, kf_node_size)
    return dict(matcher="bow", name="bow-%s-%s-nn%g" % ("rig" if rig else "mono", plan, nn), size=size, cases=cases, args=a)


def bow_scenes():
    out = []
    for rig in (False, True):
        out += [bow_scene(p, rig) for p in ("edges", "ties", "tenth2", "tenth3", None)] + [bow_scene("edges", rig, nn=1.5)]
        out += [bow_scene("edges", rig, node_size=n, kf_node_size=k) for n, k in ((63, 0), (64, 64), (65, 65), (512, 0), (513, 3))]
        out += [bow_scene(p, rig, node_size=65) for p in ("ties", "tenth2", "tenth3")] + [bow_scene("edges", rig, nn=1.5, node_size=65)]
    return out


def oracle_bow(a):
    n, m = O.search_by_bow(a["kfOff"], a["kfIdx"], a["fOff"], a["fIdx"], a["kfDesc"], a["kfAngle"], a["kfHasMP"], a["fDesc"], a["fAngle"], a["nnRatio"],
                           a["checkOrientation"], nLeft=a["nLeft"])
    return dict(n=np.int64(n), match=m)


# ======================================================================================================================
# ORBmatcher::SearchForInitialization: level-0 keypoints of frame 1 against a window of 10 pixels in frame 2
# ======================================================================================================================
INIT_WINDOW = 10


def init_scene(plan="edges", nn=0.75, pad1=0, pad2=0):
    F1, F2, cases, k = Frame(), Frame(), [], [0]

    def new_site():
        k[0] += 1
        return site(k[0] - 1) + (pattern(k[0] - 1),)

    def case(i1, gate):
        cases.append((i1, gate))

    u, v, P = new_site()
    X = flip(P, 0, 10)
    A = F1.add(u, v, 0, P); F2.add(u + 1, v, 0, X)
    case(A, "keypoint 0 of frame 1 matches at 10 ...")
    case(F1.add(u + 2, v, 0, flip(X, 100, 8)), "... a later keypoint at 8 steals the match: the entry of keypoint 0 is withdrawn")
    C = flip(X, 130, 8)
    case(F1.add(u - 2, v, 0, C), "... a third at 8 again: vMatchedDistance <= dist at equality, it must look elsewhere (25)"); F2.add(u - 1, v + 1, 0, flip(C, 160, 25))
    u, v, P = new_site()
    X2 = flip(P, 0, 10)
    A2 = F1.add(u, v, 0, P); X2i = F2.add(u + 1, v, 0, X2)
    case(A2, "a second theft: the loser's histogram entry lies in a deleted bin and must not be counted twice")
    case(F1.add(u + 2, v, 0, flip(X2, 100, 8)), "... its thief")
    u, v, P = new_site(); case(F1.add(u, v, 1, P), "frame-1 keypoint on level 1: not searched"); F2.add(u + 1, v, 1, flip(P, 0, 5))
    u, v, P = new_site(); case(F1.add(u, v, 0, P), "only a level-1 keypoint in the window: refused"); F2.add(u + 1, v, 1, flip(P, 0, 5))
    u, v, P = new_site(); case(F1.add(u, v, 0, P), "best == TH_LOW"); F2.add(u + 1, v, 0, flip(P, 0, TH_LOW))
    u, v, P = new_site(); case(F1.add(u, v, 0, P), "best == TH_LOW + 1"); F2.add(u + 1, v, 0, flip(P, 0, TH_LOW + 1))
    u, v, P = new_site(); case(F1.add(u, v, 0, P), "ratio at float equality 30 == 40 * 0.75: refused (strict <)"); F2.add(u + 1, v, 0, flip(P, 0, 40)); F2.add(u - 1, v, 0, flip(P, 60, 30))
    u, v, P = new_site(); case(F1.add(u, v, 0, P), "ratio passed (29 against 40)"); F2.add(u + 1, v, 0, flip(P, 0, 40)); F2.add(u - 1, v, 0, flip(P, 60, 29))
    u, v, P = new_site(); case(F1.add(u, v, 0, P), "tie in best: refused below ratio 1, the first visited at ratio 1.5"); F2.add(u - 7, v, 0, flip(P, 0, 20)); F2.add(u + 7, v, 0, flip(P, 40, 20))
    u, v, P = new_site(); case(F1.add(u, v, 0, P), "tie in second best"); F2.add(u - 7, v, 0, flip(P, 0, 12)); F2.add(u + 7, v, 0, flip(P, 40, 40)); F2.add(u + 7, v + 1, 0, flip(P, 90, 40))
    for axis in "xy":
        for sign in (1, -1):
            for which in (0, 1):
                u, v, P = new_site()
                pos = offset_exact(u if axis == "x" else v, f32(INIT_WINDOW), sign)[which]
                case(F1.add(u, v, 0, P), "frame-2 keypoint %s the window in %s%s" % (("exactly on the edge of", "one unit inside")[which], "+-"[sign < 0], axis))
                F2.add(pos if axis == "x" else u + 1, pos if axis == "y" else v - 1, 0, flip(P, 0, 10))
    for j in range(40):
        u, v, P = new_site(); case(F1.add(u, v, 0, P), "plain pair %d" % j); F2.add(u + 1 + j % 3, v - 1, 0, flip(P, 0, 8 + j % 5))
    kp1, d1, _, idx1 = F1.build(pad1, octave0=True, low=True)
    kp2, d2, _, idx2 = F2.build(pad2)
    a = dict(kp1=kp1, desc1=d1, kp2=kp2, desc2=d2, windowSize=INIT_WINDOW, nnRatio=nn, checkOrientation=plan is not None)
    kp1["angle"], kp2["angle"] = 0.0, 0.0
    if plan is not None:
        _, m = O.search_for_initialization(view(kp1, d1), view(kp2, d2), INIT_WINDOW, nn, False)
        plain = {idx1(i) for i, g in cases if g.startswith("plain pair")}
        pairs = sorted(np.flatnonzero(m >= 0), key=lambda i: (i in plain, i))
        for i, (a1, a2) in zip(pairs, rotation_angles(plan, len(pairs))):
            kp1["angle"][i], kp2["angle"][m[i]] = a1, a2
        # keypoint 0 lost its match, but its entry stays in the histogram, in the fullest bin (2); the loser of the second theft lies
        # in bin round(195 / 30) = 7, one of the deleted bins
        kp1["angle"][idx1(A)] = f32(kp2["angle"][idx2(0)] + f32(60.0))
        kp1["angle"][idx1(A2)] = f32(kp2["angle"][idx2(X2i)] + f32(195.0))
    size = "bare" if not (pad1 or pad2) else "padded-%d-%d" % (len(kp1), len(kp2))
    return dict(matcher="initialization", name="initialization-%s-nn%g" % (plan, nn), size=size, cases=[(idx1(i), g) for i, g in cases], args=a)


def init_scenes():
    return [init_scene(), init_scene(nn=1.5), init_scene(None), init_scene(pad1=1100, pad2=2100), init_scene(nn=1.5, pad1=1100, pad2=1300),
            init_scene(pad1=2100, pad2=600)]


def oracle_initialization(a):
    n, m = O.search_for_initialization(view(a["kp1"], a["desc1"]), view(a["kp2"], a["desc2"]), a["windowSize"], a["nnRatio"], a["checkOrientation"])
    return dict(n=np.int64(n), matches12=m)


# ======================================================================================================================
# ORBmatcher::SearchForTriangulation, its own gates (pinhole pair).  F12 is chosen so that the epipolar line of a key-frame-1
# keypoint is the image row through it: a = 0, b = 1, c = -y1, so the squared distance of the test is (y2 - y1)^2 exactly.
# ======================================================================================================================
TRI_F12 = (0, 0, 0, 0, 0, -1, 0, 1, 0)
TRI_EP = (MINX + 20.0, MINY + 20.0)


def tri_scene(only_stereo=False, node_size=0, kb8=False):
    K1, K2, groups, cases, k = Frame(), Frame(), [], [], [0]

    def new_site():
        k[0] += 1
        return site(k[0]) + (pattern(k[0]),)     # site 0 is next to the epipole: left free

    def group(one, twos, gate):
        """one: (x, y, octave, desc, hasMP, stereo); twos: the same for key frame 2, in the node's list order"""
        i1 = K1.add(*one[:4], has=one[4], stereo=one[5])
        groups.append(([i1], [K2.add(*t[:4], has=t[4], stereo=t[5]) for t in twos]))
        cases.append((i1, gate))

    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v, 0, flip(P, 0, TH_LOW), 0, 0)], "distance == TH_LOW: matched -- with feature 0 of key frame 2")
    u, v, P = new_site(); group((u, v, 0, P, 1, 0), [(u + 8, v, 0, flip(P, 0, 5), 0, 0)], "key-frame-1 feature has a map point")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v, 0, flip(P, 0, 5), 1, 0)], "the only candidate has a map point")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v, 0, flip(P, 0, TH_LOW + 1), 0, 0)], "distance == TH_LOW + 1: refused")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v + 0.5, 0, flip(P, 0, 20), 0, 0), (u + 10, v - 0.5, 0, flip(P, 40, 20), 0, 0)], "tie: the LATER of equal distances wins here")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v, 0, flip(P, 0, 25), 0, 0), (u + 10, v, 0, flip(P, 40, 20), 0, 0)], "later and nearer")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v, 0, flip(P, 0, 20), 0, 0), (u + 10, v, 0, flip(P, 40, 25), 0, 0)], "later and farther")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v + 1.9, 0, flip(P, 0, 10), 0, 0)], "1.9 pixels off the epipolar line: 3.61 < 3.84")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v + 2.0, 0, flip(P, 0, 10), 0, 0)], "2 pixels off the epipolar line: refused")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 8, v + 3, 0, flip(P, 0, 10), 0, 0), (u + 10, v, 0, flip(P, 40, 20), 0, 0)], "the nearer descriptor is off the line: it must not lower the bar")
    u, v, P = new_site(); group((u, v, 0, P, 0, 0), [(u + 10, v, 0, flip(P, 40, 20), 0, 0), (u + 8, v + 3, 0, flip(P, 0, 10), 0, 0)], "the same, the other way round")
    # the epipolar gate at its constant: 3.84f lies BELOW the double 3.84, so a squared distance of exactly 3.84f passes `< 3.84` and fails
    # `< 3.84f`.  SearchForTriangulation has no image bounds, so the pair sits at y1 = 2^-6 and y2 in [1, 2), where y2 - y1 is exact
    # and has steps of 2^-23: one of them squares to 3.84f exactly
    step, y1 = 2.0 ** -23, f32(2.0 ** -6)
    k0 = int(round(np.sqrt(3.84) / step))
    sq = lambda kk: f32(f32(kk * step) * f32(kk * step))
    on = [f32(kk * step) for kk in range(k0 - 8, k0 + 8) if sq(kk) == f32(3.84)]
    above = next(f32(kk * step) for kk in range(k0, k0 + 8) if sq(kk) > f32(3.84))
    assert on and np.float64(f32(3.84)) < 3.84 and f32(f32(y1 + on[0]) - y1) == on[0] and f32(f32(y1 + above) - y1) == above
    P = pattern(88)
    group((3.0, y1, 0, P, 0, 0), [(3.5, f32(y1 + on[0]), 0, flip(P, 0, 10), 0, 0)], "squared epipolar distance == 3.84f exactly: below the double 3.84, kept")
    P = pattern(89)
    group((5.0, y1, 0, P, 0, 0), [(5.5, f32(y1 + above), 0, flip(P, 0, 10), 0, 0)], "squared epipolar distance one step above 3.84f: refused")
    ex, ey = f32(TRI_EP[0]), f32(TRI_EP[1])
    P = pattern(90)
    group((ex + 30, ey + 8, 0, P, 0, 0), [(ex + 6, ey + 8, 0, flip(P, 0, 10), 0, 0)], "squared distance to the epipole == 100 * sf[0] exactly: kept (strict <)")
    P = pattern(91)
    group((ex + 30, ey + 7.5, 0, P, 0, 0), [(ex + 6, ey + 7.5, 0, flip(P, 0, 10), 0, 0)], "92.25 from the epipole: dropped")
    P = pattern(92)
    group((ex + 30, ey + 7.25, 0, P, 0, 0), [(ex + 6, ey + 7.25, 0, flip(P, 0, 10), 0, 1)], "near the epipole but stereo in key frame 2: no epipole gate")
    P = pattern(93)
    group((ex + 30, ey + 7, 0, P, 0, 1), [(ex + 6, ey + 7, 0, flip(P, 0, 10), 0, 0)], "near the epipole but stereo in key frame 1: no epipole gate")
    P = pattern(94)
    group((ex + 30, ey - 8, 0, P, 0, 0), [(ex + 6, ey - 8, 1, flip(P, 0, 10), 0, 0)], "100 from the epipole on level 1 of key frame 2: 100 < 120, dropped")
    P = pattern(95)
    group((ex + 30, ey - 7, 1, P, 0, 0), [(ex + 8, ey - 7, 0, flip(P, 0, 10), 0, 0)], "113 from the epipole, key-frame-1 keypoint on level 1: the scale is key frame 2's, kept")
    for j in range(56):
        u, v, P = new_site(); group((u, v, 0, P, 0, j % 2), [(u + 8, v + 0.25 * (j % 4), 0, flip(P, 0, 8 + j % 5), 0, j % 2)], "plain pair %d" % j)
    # padded: inert features (far descriptors; with a map point on the key-frame-1 side) around the planted ones in every node
    off1, idx1, off2, idx2 = [0], [], [0], []
    for g, (ones, twos) in enumerate(groups):
        pad = max(0, node_size - len(twos))
        extra1 = [K1.add(MINX + 4 + (g * 7 + j) % 500, MAXY - 20, 0, Frame.filler(g * 3 + j)["desc"], has=1, stereo=0) for j in range(min(pad, 3))]
        extra2 = [K2.add(MINX + 4 + (g * 7 + j) % 500, MAXY - 20, 0, Frame.filler(g * 5 + j)["desc"], has=0, stereo=j % 2) for j in range(pad)]
        idx1 += extra1[:1] + ones + extra1[1:]
        idx2 += extra2[:pad // 2] + twos + extra2[pad // 2:]
        off1.append(len(idx1)); off2.append(len(idx2))
    kp1, d1, e1, _ = K1.build(defaults=dict(has=0, stereo=0))
    kp2, d2, e2, _ = K2.build(defaults=dict(has=0, stereo=0))
    a = dict(off1=np.array(off1, np.int32), idx1=np.array(idx1, np.int32), off2=np.array(off2, np.int32), idx2=np.array(idx2, np.int32), kp1=kp1, desc1=d1,
             hasMP1=e1["has"].astype(np.uint8), stereo1=e1["stereo"].astype(np.uint8), kp2=kp2, desc2=d2, hasMP2=e2["has"].astype(np.uint8),
             stereo2=e2["stereo"].astype(np.uint8), scaleFactors2=SF, F12=np.array(TRI_F12, np.float32), ep=TRI_EP, bOnlyStereo=only_stereo, bCoarse=False,
             checkOrientation=True, cameras=None)
    if kb8:   # two KannalaBrandt8 cameras without distortion terms, 0.1 to the side of each other: a disparity of 8 pixels is 0.03 rad of parallax
        cam = (FX, FY, CX, CY, 0.0, 0.0, 0.0, 0.0)
        a["cameras"] = dict(model1=1, model2=1, cam1=cam, cam2=cam, precision=1e-6, R12=np.eye(3, dtype=np.float32), t12=np.array((-0.1, 0, 0), np.float32),
                            levelSigma2_1=(SF * SF).astype(np.float32), kf1HasCamera2=0)
    kp1["angle"], kp2["angle"] = 0.0, 0.0
    _, m = oracle_triangulation(dict(a, checkOrientation=False)).values()
    plain = {i for i, g in cases if g.startswith("plain pair")}
    pairs = sorted(np.flatnonzero(m >= 0), key=lambda i: (i in plain, i))
    for i, (a1, a2) in zip(pairs, rotation_angles("edges", len(pairs))):
        kp1["angle"][i], kp2["angle"][m[i]] = a1, a2
    return dict(matcher="triangulation", name="triangulation%s%s" % ("-kb8" if kb8 else "", "-onlystereo" if only_stereo else ""), size="bare" if not node_size else "padded-node%d" % node_size,
                cases=cases, args=a)


def oracle_triangulation(a):
    n, m = O.search_for_triangulation(a["off1"], a["idx1"], a["off2"], a["idx2"], a["kp1"], a["desc1"], a["hasMP1"], a["stereo1"], a["kp2"], a["desc2"],
                                      a["hasMP2"], a["stereo2"], a["scaleFactors2"], a["F12"], a["ep"], a["bOnlyStereo"], a["bCoarse"], a["checkOrientation"], cameras=a["cameras"])
    return dict(n=np.int64(n), matches12=m)


ORACLE = {"projection": oracle_projection, "fuse": oracle_fuse, "fuse_right": oracle_fuse_right, "fuse_sim3": oracle_fuse_sim3, "bow": oracle_bow, "frustum": oracle_frustum, "projection_kf": oracle_projection_kf, "sim3": oracle_sim3, "initialization": oracle_initialization, "triangulation": oracle_triangulation}


def scenes():
    """every planted scene at every size"""
    out = [projection_scene(), projection_scene(1300, 300), projection_scene(2100, 1000)]
    out += fuse_scenes() + fuse_scenes(1200, 300) + fuse_scenes(2000, 1000)
    out += bow_scenes()
    out += [frustum_scene(), frustum_scene(5000)]
    out += init_scenes()
    out += [tri_scene(), tri_scene(True), tri_scene(node_size=64), tri_scene(node_size=65), tri_scene(True, node_size=65),
            tri_scene(kb8=True), tri_scene(kb8=True, node_size=65)]
    return out


def run_oracle(scene):
    """the arrays the GPU test compares, from whichever library oracle_py is bound to"""
    return ORACLE[scene["matcher"]](scene["args"])
