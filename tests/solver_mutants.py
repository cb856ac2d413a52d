"""One-token mutants of the solver restatements' own Python text and their loader (helper module of tests/test_solver_gates.py, not
a test), in the manner of tests/gate_mutants.py.

Every solver kernel is compared with its numpy restatement byte for byte; that comparison sees a kernel mistake only on a scene where
the mistake changes an output.  Each entry of MUTANTS is such a mistake written into the restatement: a gate made lax or strict, a
cast dropped, a product taken in the wrong width, a tie broken the other way.  tests/test_solver_gates.py proves that the scenes of
tests/solver_gates.py tell every mutant from the real restatement; tests/test_solver_gates_gpu.py then runs the library on them.

An entry: module, function, anchor -- a string that occurs exactly once in that function --, replacement, the kernel mistake it
stands for, equivalence argument or None, and `families`: which scene families run it and how the mutated function reaches that
family's restatement (ROUTES).  An entry with an argument is asserted NOT to differ on any scene.

The loader reads the module's source, replaces the anchor, compiles the text and executes it into a fresh module object.  Nothing is
written to disk and sys.modules is left alone.

Kernel-shaped mistakes that have no counterpart in a restatement's text, and the scene of tests/solver_gates.py that catches each:

  mistake                                            scene(s)                          why
  -------------------------------------------------  --------------------------------  -----------------------------------------------
  twoview_select_kernel: the lower LANE wins the     twoview *-lower_iteration_higher_ the equal maxima sit at iterations 10 (lane 10)
  cross-lane reduction, not the lower iteration      lane                              and 69 (lane 5): lane order returns 69
  ... the higher lane wins                           twoview *-lower_iteration_lower_  iterations 5 (lane 5) and 74 (lane 10): returns 74
                                                     lane
  ... a lane keeps the last of its equals            twoview *-same_lane, *-four_      iterations 37 / 101, and 7 / 71 / 135 / 199, are
                                                     strides                           one lane's own: returns 101 or 199
  mlpnp_refine_kernel: the strided `beaten` loop     mlpnp copies_in_second_trip       the largest count occurs at iterations 260 and 286
  (j = tid; j < it; j += 256) stops after one trip                                     only: 286 is beaten by nothing below 256 and would
                                                                                       become a candidate
  pose_opt_frame<1 / 2 / 4>: act[k] (the flag kept   poseopt *-N12-*, *-N257-* with a  the tied edge stays active in the restatement; a
  in registers) not refreshed after a round          tie in round 0, 1 or 2            stale or wrongly refreshed flag changes the sums
                                                                                       of the next round, so its pose, lambda and chi2
  pose_opt_frame<0>: F.outlier read back stale       poseopt *-N1025-* with a tie in   the same, through the flags in memory: at
  (the write of the round before not yet visible)    round 0, 1 or 2                   N_e = 1025 an edge's flag is written by one thread
                                                                                       of the scoring pass and read by the next build
"""
import os
import re
import types

HERE = os.path.dirname(os.path.abspath(__file__))

M = []


def _m(module, fn, anchor, repl, what, families, equivalent=None):
    M.append(dict(id="%s.%s#%02d" % (module, fn, sum(1 for m in M if (m["module"], m["fn"]) == (module, fn))), module=module, fn=fn,
                  anchor=anchor, repl=repl, what=what, families=families, equivalent=equivalent))


# how a mutated module reaches a family's restatement: the names injected into fresh copies of the modules downstream
SELF = ()
ROBUST_R19 = (("pose_inertial_ref", "robust"),)                                     # poseopt_ref.robust as pose_inertial_ref uses it
ROBUST_R19_R20 = (("pose_inertial_ref", "robust"), ("pose_inertial_prev_ref", "R19"))   # ... and S20's mono edges through it
ROBUST_R20 = (("pose_inertial_prev_ref", "robust"),)                                # S20's prior edge only
R19_R20 = (("pose_inertial_prev_ref", "R19"),)                                      # pose_inertial_ref as pose_inertial_prev_ref uses it

HUBER = ("wherever chi2 == delta * delta exactly, sqrt(chi2) == delta (a correctly rounded square root returns the root of a rounded "
         "square), so the linear branch gives rho0 = 2 delta delta - delta delta = chi2 and rho1 = delta / delta = 1: both branches agree; "
         "elsewhere `<=` and `<` do not differ")

# ---- S14: Optimizer::PoseOptimization ------------------------------------------------------------------------------------
P = dict(poseopt=SELF)
_m("poseopt_ref", "pose_optimization", ".astype(np.float32) > thr", ".astype(np.float32) >= thr", "an edge whose chi2 equals chi2_threshold flagged", P)
_m("poseopt_ref", "pose_optimization", "chi2_of(e0, e1, w).astype(np.float32) > thr", "chi2_of(e0, e1, w) > thr",
   "the float cast of chi2 dropped: the binary64 chi2 compared with the threshold", P)
_m("poseopt_ref", "pose_optimization", "rnd <= 2", "rnd < 2", "the Huber kernel dropped one round early", P)
_m("poseopt_ref", "pose_optimization", "rnd <= 2", "rnd <= 3", "the Huber kernel kept in the last round", P)
_m("poseopt_ref", "robust", "small = chi2 <= d2", "small = chi2 < d2", "Huber's quadratic region without its end point",
   dict(poseopt=SELF, inertial=ROBUST_R19, inertial_prev=ROBUST_R19_R20), equivalent=HUBER)
_m("poseopt_ref", "robust", "small = chi2 <= d2", "small = chi2 < d2", "the prior's Huber (S20) without the end point of its quadratic region",
   dict(inertial_prev=ROBUST_R20), equivalent=HUBER)

# ---- S19 / S20: the gates both restatements write out, and imu_edge_is_outlier's callers -----------------------------------
for mod, fn, fam in (("pose_inertial_ref", "pose_inertial_optimization", dict(inertial=SELF)),
                     ("pose_inertial_prev_ref", "pose_inertial_optimization_last_frame", dict(inertial_prev=SELF))):
    _m(mod, fn, "(chi2 > thr) & ~close", "(chi2 >= thr) & ~close", "a far edge whose chi2 equals chi2[round] flagged", fam)
    _m(mod, fn, "close & (chi2 > thr_close)", "close & (chi2 >= thr_close)", "a close edge whose chi2 equals its bound flagged", fam)
    _m(mod, fn, "(chi2 > thr) & ~close", "(chi2 > thr) & close", "the plain threshold applied to the close edges", fam)
    _m(mod, fn, "(close & (chi2 > thr_close))", "(~close & (chi2 > thr_close))", "the close bound applied to the far edges", fam)
    _m(mod, fn, " | ~front", "", "an edge with Xc.z <= 0 flagged only by its chi2: a NaN chi2 passes", fam)
    _m(mod, fn, 'f32(f64(prm["close_factor"]) * f64(thr))', '(f32(prm["close_factor"]) * thr)', "the close bound computed in binary32", fam)
    _m(mod, fn, "rnd <= 2", "rnd < 2", "the Huber kernel dropped one round early", fam)
    _m(mod, fn, "rnd <= 2", "rnd <= 3", "the Huber kernel kept in the last round", fam)
    _m(mod, fn, '< f32(prm["close_depth"])', '<= f32(prm["close_depth"])', "a point exactly close_depth away counted as close", fam)
    _m(mod, fn, 'Ne - n_bad < prm["recover_below"]', 'Ne - n_bad <= prm["recover_below"]', "recovery with exactly recover_below inliers left", fam)
    _m(mod, fn, 'good = chi2 < f32(prm["recover_chi2"])', 'good = chi2 <= f32(prm["recover_chi2"])', "an edge whose chi2 equals recover_chi2 taken back", fam)
    _m(mod, fn, "bad = bad & ~good", "bad = ~good", "the recovery pass flags every edge that is not good, not only the flagged ones", fam)
    _m(mod, fn, "n_bad = int((~good).sum())", "n_bad = int(bad.sum())", "the recovery pass counts the flags, not the edges that are not good", fam)
B = dict(inertial=SELF, inertial_prev=R19_R20)
_m("pose_inertial_ref", "score", "z > 0.0", "z >= 0.0", "an edge at depth exactly 0 counted as in front of the camera", B)
_m("pose_inertial_ref", "score", "chi2_of(e0, e1, w).astype(f32), z", "chi2_of(e0, e1, w), z", "the float cast of chi2 dropped", B)

# ---- S12: the winner among the hypotheses ------------------------------------------------------------------------------------
T = dict(twoview=SELF)
_m("twoview_ref", "first_max", "if s > best:", "if s >= best:", "the last of equal scores wins (and a score of 0 wins over no hypothesis)", T)
_m("twoview_ref", "first_max", "in enumerate(scores):", "in reversed(list(enumerate(scores))):", "the winner loop runs from the last iteration", T)

# ---- S13: candidates, the returning rule, the inlier test ------------------------------------------------------------------
L = dict(mlpnp=SELF)
_m("mlpnp_ref", "_ransac", "and cnt[i] > best:", "and cnt[i] >= best:", "a hypothesis that only equals an earlier count becomes a candidate "
   "(the kernel's `hypCount[j] >= mine` as `>`)", L)
_m("mlpnp_ref", "_ransac", "if cnt[i] >= nMin and", "if cnt[i] > nMin and", "a hypothesis with exactly mRansacMinInliers inliers does not qualify", L)
_m("mlpnp_ref", "_ransac", "int(m.sum()) > nMin", "int(m.sum()) >= nMin", "a refined pose with exactly mRansacMinInliers inliers returns", L)
_m("mlpnp_ref", "check_inliers", "(e2 < np.tile", "(e2 <= np.tile", "an error exactly on mvMaxError counted as an inlier", L)

MUTANTS = M


def function_span(text, name):
    """(start, end) of the top-level function `name` in a module's text: from its `def` to the next line that starts a top-level
    statement"""
    m = re.search(r"^def %s\(" % re.escape(name), text, re.M)
    if not m:
        raise ValueError("function %s not found" % name)
    nxt = re.compile(r"^[^\s#)]", re.M).search(text, m.end())
    return m.start(), nxt.start() if nxt else len(text)


def mutate(text, mutant):
    a, b = function_span(text, mutant["fn"])
    n = text[a:b].count(mutant["anchor"])
    if n != 1:
        raise ValueError("mutant %s: anchor %r occurs %d times in %s (must be exactly once)" % (mutant["id"], mutant["anchor"], n, mutant["fn"]))
    return text[:a] + text[a:b].replace(mutant["anchor"], mutant["repl"]) + text[b:]


def source(module):
    with open(os.path.join(HERE, module + ".py")) as f:
        return f.read()


def execute(module, text, inject=None):
    """the text as a fresh module object; `inject` replaces names after the execution (the functions look them up when called)"""
    path = os.path.join(HERE, module + ".py")
    mod = types.ModuleType(module + "__mutant")
    mod.__file__ = path
    exec(compile(text, path, "exec"), mod.__dict__)
    for k, v in (inject or {}).items():
        assert k in mod.__dict__, (module, k)
        setattr(mod, k, v)
    return mod


def load(mutant, family):
    """the restatement of `family` with the mutant in it"""
    mod = execute(mutant["module"], mutate(source(mutant["module"]), mutant))
    for module, name in mutant["families"][family]:
        mod = execute(module, source(module), {name: getattr(mod, name) if name == mutant["fn"] else mod})
    return mod


def control(family, module):
    """the unmutated text through the same loader"""
    return execute(module, source(module))
