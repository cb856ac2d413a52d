"""One-token mutants of oracle/match_oracle.c and their builder (helper module of tests/test_gate_scenes.py, not a test).

Every GPU matcher is compared with the oracle byte for byte; that comparison sees a kernel mistake only on a scene where
the mistake changes an output.  Each entry of MUTANTS is such a mistake written into the oracle's own text: a gate made
lax or strict, a floor that should be a ceil, a constant of the wrong width, a deleted `continue`, a tie broken the other
way.  tests/test_gate_scenes.py proves that the planted scenes of tests/gate_scenes.py tell every mutant from the real
oracle; tests/test_gate_scenes_gpu.py then runs the library on those scenes.

An entry: (oracle function, anchor -- a string that occurs exactly once in that function --, replacement, the kernel mistake
it stands for, equivalence argument or None).  An entry with an argument is asserted NOT to differ on any scene."""
import atexit
import concurrent.futures
import os
import re
import shutil
import subprocess
import tempfile

import oracle_py as O

SOURCE = os.path.join(O.ODIR, "match_oracle.c")
OTHERS = ("orb_oracle.c", "prep_oracle.c")
MAX_JOBS = 8

LOOPS = ("for (int ix = nMinCellX; ix <= nMaxCellX; ix++)\n        for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {",
         "for (int iy = nMinCellY; iy <= nMaxCellY; iy++)\n        for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {")

# which scenes (tests/gate_scenes.py: scene["matcher"]) run a function of the oracle
SCENES_OF = {
    "pos_in_grid": ("projection", "initialization", "fuse", "fuse_right", "fuse_sim3", "sim3", "projection_kf"),
    "features_in_area": ("projection", "initialization", "fuse", "fuse_right", "fuse_sim3", "sim3", "projection_kf"),
    "radius_by_viewing_cos": ("projection",),
    "orc_search_by_projection": ("projection",),
    "compute_three_maxima": ("bow", "initialization", "projection_kf", "triangulation"),
    "orc_search_by_bow_rig": ("bow",),
    "orc_search_for_initialization": ("initialization",),
    "orc_is_in_frustum": ("frustum",),
    "fuse_search_body": ("fuse", "fuse_right", "fuse_sim3"),
    "predict_scale": ("sim3", "projection_kf"),
    "sim3_direction": ("sim3",),
    "orc_search_by_sim3": ("sim3",),
    "orc_search_by_projection_kf": ("projection_kf",),
    "orc_search_for_triangulation_cam": ("triangulation",),
}

M = []


def _m(fn, anchor, repl, what, equivalent=None):
    M.append(dict(id="%s#%02d" % (fn, sum(1 for m in M if m["fn"] == fn)), fn=fn, anchor=anchor, repl=repl, what=what,
                  equivalent=equivalent))


# ---- Frame::PosInGrid ------------------------------------------------------------------------------------------------
_m("pos_in_grid", "roundf((kp->x", "floorf((kp->x", "cell column by truncation instead of rounding")
_m("pos_in_grid", "roundf((kp->y", "floorf((kp->y", "cell row by truncation instead of rounding")
_m("pos_in_grid", "linearIdx >= 0", "linearIdx > 0", "cell (0, 0) treated as outside the grid")
# `linearIdx < size` -> `<=` is not here: its only effect is a write one cell past the grid, which no output array shows.

# ---- Frame::GetFeaturesInArea ----------------------------------------------------------------------------------------
_m("features_in_area", "floorf((x - F->minX - factorX)", "ceilf((x - F->minX - factorX)", "low cell column rounded up: the partly covered column is lost")
_m("features_in_area", "ceilf((x - F->minX + factorX)", "floorf((x - F->minX + factorX)", "high cell column rounded down")
_m("features_in_area", "floorf((y - F->minY - factorY)", "ceilf((y - F->minY - factorY)", "low cell row rounded up")
_m("features_in_area", "ceilf((y - F->minY + factorY)", "floorf((y - F->minY + factorY)", "high cell row rounded down")
_m("features_in_area", "floorf((x - F->minX - factorX)", "truncf((x - F->minX - factorX)", "low cell column truncated toward zero",
   equivalent="truncf and floorf differ only below zero, and a negative low cell is clamped to 0 on the next line either way")
_m("features_in_area", "ceilf((x - F->minX + factorX)", "1.0f + floorf((x - F->minX + factorX)", "high cell column as floor + 1",
   equivalent="differs only when the window edge lies exactly on a cell boundary k: the extra column k + 1 holds keypoints whose rounded "
              "cell is k + 1, so they lie at least half a cell beyond the edge and fail |dx| < r")
_m("features_in_area", "floorf((y - F->minY - factorY)", "truncf((y - F->minY - factorY)", "low cell row truncated toward zero",
   equivalent="as for the column: truncf and floorf differ only below zero, and a negative low row is clamped to 0 on the next line")
_m("features_in_area", "ceilf((y - F->minY + factorY)", "1.0f + floorf((y - F->minY + factorY)", "high cell row as floor + 1",
   equivalent="as for the column: the extra row k + 1 holds keypoints at least half a cell beyond the window edge, which fail |dy| < r")
_m("features_in_area", "nMinCellY >= F->gridRows", "nMinCellY > F->gridRows", "window starting one row past the grid not refused",
   equivalent="with nMinCellY == gridRows the high row is clamped to gridRows - 1 and the row loop runs zero times")
_m("features_in_area", "nMaxCellX < 0", "nMaxCellX <= 0", "a window whose last column is column 0 dropped")
_m("features_in_area", "nMaxCellY < 0", "nMaxCellY <= 0", "a window whose last row is row 0 dropped")
_m("features_in_area", "nMinCellX >= F->gridCols", "nMinCellX > F->gridCols", "window starting one column past the grid not refused",
   equivalent="with nMinCellX == gridCols the high column is clamped to gridCols - 1 and the column loop runs zero times")
_m("features_in_area", "ix <= nMaxCellX", "ix < nMaxCellX", "last cell column of the window not visited")
_m("features_in_area", "iy <= nMaxCellY", "iy < nMaxCellY", "last cell row of the window not visited")
_m("features_in_area", LOOPS[0], LOOPS[1], "cells visited row by row instead of column by column: another first among equal distances")
_m("features_in_area", "(maxLevel >= 0);", "(maxLevel > 0);", "level check switched off for a level-0 query")
_m("features_in_area", "kpUn->octave < minLevel", "kpUn->octave <= minLevel", "the lower level of the pair excluded")
_m("features_in_area", "(maxLevel >= 0 && kpUn", "(maxLevel > 0 && kpUn", "no upper level bound for a level-0 query")
_m("features_in_area", "kpUn->octave > maxLevel", "kpUn->octave >= maxLevel", "the upper level of the pair excluded")
_m("features_in_area", "kpUn->octave > maxLevel)) continue;", "kpUn->octave > maxLevel)) {}", "level gate deleted")
_m("features_in_area", "fabsf(distx) < factorX", "fabsf(distx) <= factorX", "keypoint exactly r away in x accepted")
_m("features_in_area", "fabsf(disty) < factorY", "fabsf(disty) <= factorY", "keypoint exactly r away in y accepted")

# ---- ORBmatcher::SearchByProjection (Frame, map points) ----------------------------------------------------------------
_m("radius_by_viewing_cos", "viewCos > 0.998 ?", "viewCos > 0.998f ?", "float constant 0.998f: a cosine of exactly 0.998f gets the wide radius")
_m("orc_search_by_projection", "if (!pMP->inView) continue;", "", "points outside the frustum searched")
_m("orc_search_by_projection", "pMP->trackDepth > thFarPoints", "pMP->trackDepth >= thFarPoints", "a point exactly at the far threshold dropped")
_m("orc_search_by_projection", "if (bFarPoints && pMP->trackDepth > thFarPoints) continue;", "", "far-point gate deleted")
_m("orc_search_by_projection", "if (pMP->bad) continue;", "", "bad points searched")
_m("orc_search_by_projection", "nPredictedLevel - 1, nPredictedLevel, vIndices", "nPredictedLevel, nPredictedLevel, vIndices", "level pair without lvl - 1")
_m("orc_search_by_projection", "nPredictedLevel - 1, nPredictedLevel, vIndices", "nPredictedLevel - 1, nPredictedLevel + 1, vIndices", "level pair widened to lvl + 1")
_m("orc_search_by_projection", "slotObs[idx] > 0", "slotObs[idx] >= 0", "a keypoint whose map point has 0 observations counts as taken")
_m("orc_search_by_projection", "if (slotObs[idx] > 0) continue;", "", "taken keypoints compete")
_m("orc_search_by_projection", "dist < bestDist)", "dist <= bestDist)", "the last of equal best distances wins")
_m("orc_search_by_projection", "dist < bestDist2)", "dist <= bestDist2)", "the last of equal second-best distances sets bestLevel2")
_m("orc_search_by_projection", "bestLevel = F->kp[idx].octave;", "bestLevel = nPredictedLevel;", "bestLevel taken from the prediction, not the keypoint")
_m("orc_search_by_projection", "bestLevel2 = bestLevel;", "bestLevel2 = F->kp[idx].octave;", "bestLevel2 not inherited from the dethroned best")
_m("orc_search_by_projection", "bestLevel2 = F->kp[idx].octave;", "bestLevel2 = nPredictedLevel;", "bestLevel2 taken from the prediction")
_m("orc_search_by_projection", "bestDist <= TH_HIGH", "bestDist < TH_HIGH", "a best distance of exactly TH_HIGH refused")
_m("orc_search_by_projection", "(float)bestDist > nnRatio * (float)bestDist2) continue;", "(float)bestDist >= nnRatio * (float)bestDist2) continue;", "ratio test refuses equality")
_m("orc_search_by_projection", "(float)bestDist <= nnRatio * (float)bestDist2)", "(float)bestDist < nnRatio * (float)bestDist2)", "ratio test (second form) refuses equality")
_m("orc_search_by_projection", "bestLevel != bestLevel2 ||", "", "no escape from the ratio test when the two best lie on different levels")
_m("orc_search_by_projection", "slotObs[bestIdx] = pMP->observations;", "", "a matched keypoint stays free for later points")
_m("orc_search_by_projection", "slotObs[bestIdx] = pMP->observations;", "slotObs[bestIdx] = 1;", "a keypoint matched by a point with 0 observations counts as taken")

# ---- the search part of ORBmatcher::Fuse (three callers) ---------------------------------------------------------------
B = "fuse_search_body"
_m(B, "p->skip || p->bad", "p->bad", "points already in the key frame searched")
_m(B, "p->skip || p->bad", "p->skip", "bad points searched")
_m(B, "if (pcz < 0.0f) continue; /* :725 */", "", "points behind the camera projected")
_m(B, "pcz < 0.0f", "pcz <= 0.0f", "depth 0 refused before the projection",
   equivalent="at depth 0 the projection is infinite or NaN and fails IsInImage on the next gate, so the point is dropped either way")
_m(B, "u >= F->minX", "u > F->minX", "a projection exactly on minX refused")
_m(B, "u < F->maxX", "u <= F->maxX", "a projection exactly on maxX accepted")
_m(B, "v >= F->minY", "v > F->minY", "a projection exactly on minY refused")
_m(B, "v < F->maxY", "v <= F->maxY", "a projection exactly on maxY accepted")
_m(B, "if (!(u >= F->minX && u < F->maxX && v >= F->minY && v < F->maxY)) continue;", "", "image-bounds gate deleted")
_m(B, "dist3D < minD", "dist3D <= minD", "a distance of exactly 0.9f * minDistance refused")
_m(B, "dist3D > maxD", "dist3D >= maxD", "a distance of exactly 1.1f * maxDistance refused")
_m(B, "if (dist3D < minD || dist3D > maxD) continue;", "", "distance gate deleted")
_m(B, "1.1f * p->maxDistance", "(float)(1.1 * p->maxDistance)", "1.1 as a double constant")
_m(B, "0.9f * p->minDistance", "(float)(0.9 * p->minDistance)", "0.9 as a double constant")
_m(B, "!(q > 0.0f)", "!(q >= 0.0f)", "q == 0 sent down the ceil path", equivalent="q == 0 gives level 0 either way: ceilf(0) is 0")
_m(B, "q >= (float)F->nLevels", "q > (float)F->nLevels", "q == nLevels sent down the ceil path",
   equivalent="q == nLevels gives ceilf(q) == nLevels, which the clamp on the next line turns into nLevels - 1 as well")
_m(B, "lvl = (int)ceilf(q);", "lvl = (int)floorf(q) + 1;", "ceil written as floor + 1: one level too high when q is an integer")
_m(B, "lvl = (int)ceilf(q);", "lvl = (int)roundf(q);", "level by rounding")
_m(B, "if (lvl >= F->nLevels) lvl", "if (lvl > F->nLevels) lvl", "level nLevels not clamped")
_m(B, "kpLevel < lvl - 1", "kpLevel <= lvl - 1", "level lvl - 1 excluded")
_m(B, "kpLevel < lvl - 1", "kpLevel < lvl - 2", "level lvl - 2 included")
_m(B, "kpLevel > lvl)", "kpLevel >= lvl)", "level lvl excluded")
_m(B, "kpLevel > lvl)", "kpLevel > lvl + 1)", "level lvl + 1 included")
_m(B, "if (kpLevel < lvl - 1 || kpLevel > lvl) continue;", "", "level gate deleted")
_m(B, "uRight[idx] >= 0", "uRight[idx] > 0", "uRight == 0 taken for a monocular keypoint")
_m(B, "invLevelSigma2[kpLevel] > 7.8)", "invLevelSigma2[kpLevel] > 7.8f)", "stereo gate against the float constant: 7.8f itself passes")
_m(B, "invLevelSigma2[kpLevel] > 7.8)", "invLevelSigma2[lvl] > 7.8)", "stereo gate with the sigma of the predicted level")
_m(B, "invLevelSigma2[kpLevel] > 7.8) continue;", "invLevelSigma2[kpLevel] > 7.8) {}", "stereo gate deleted")
_m(B, "invLevelSigma2[kpLevel] > 5.99)", "invLevelSigma2[kpLevel] >= 5.99f)", "mono gate refuses 5.99f, which lies below the double 5.99")
_m(B, "invLevelSigma2[kpLevel] > 5.99)", "invLevelSigma2[kpLevel] > 5.99f)", "mono gate against the float constant",
   equivalent="5.99f is the binary32 number just below the double 5.99, so for a binary32 product `> 5.99` and `> 5.99f` both mean "
              "`>= the number after 5.99f`; the stereo constant is the other way round (7.8f > 7.8) and is not equivalent")
_m(B, "invLevelSigma2[kpLevel] > 5.99)", "invLevelSigma2[lvl] > 5.99)", "mono gate with the sigma of the predicted level")
_m(B, "invLevelSigma2[kpLevel] > 5.99) continue;", "invLevelSigma2[kpLevel] > 5.99) {}", "mono gate deleted")
_m(B, "(ex * ex + ey * ey) + er * er", "ex * ex + (ey * ey + er * er)", "stereo error summed in another order")
_m(B, "idx >= nRight", "idx > nRight", "the first left feature without a right twin compared with the row past the matrix")
_m(B, "row = idx + KF->n;", "row = idx;", "bRight compares the left row")
_m(B, "bestIdx = row;", "bestIdx = idx;", "bRight returns the left index")
_m(B, "dist < bestDist)", "dist <= bestDist)", "the last of equal distances wins")

# ---- ComputeThreeMaxima ------------------------------------------------------------------------------------------------
T = "compute_three_maxima"
_m(T, "s > max1", "s >= max1", "the later of two equally full bins takes first place")
_m(T, "s > max2", "s >= max2", "the later of equally full bins takes second place")
_m(T, "s > max3", "s >= max3", "the later of equally full bins takes third place")
_m(T, "(float)max2 < 0.1f * (float)max1", "(float)max2 <= 0.1f * (float)max1", "second bin dropped at exactly a tenth of the first")
_m(T, "(float)max3 < 0.1f * (float)max1", "(float)max3 <= 0.1f * (float)max1", "third bin dropped at exactly a tenth of the first")

# ---- ORBmatcher::SearchByBoW -------------------------------------------------------------------------------------------
W = "orc_search_by_bow_rig"
_m(W, "if (!kfHasMP[realIdxKF]) continue;", "", "key-frame features without a map point matched")
_m(W, "matchOut[realIdxF] >= 0", "matchOut[realIdxF] > 0", "a frame feature matched to key-frame feature 0 counts as free")
_m(W, "if (matchOut[realIdxF] >= 0) continue;", "", "matched frame features compete again")
_m(W, "realIdxF < nLeft", "realIdxF <= nLeft", "the first right feature counted to the left camera")
_m(W, "dist < bestDist1)", "dist <= bestDist1)", "the last of equal best distances wins (left)")
_m(W, "dist < bestDist2)", "dist <= bestDist2)", "second best replaced by an equal distance (left)",
   equivalent="bestDist2 is only a value: replacing it by an equal value changes nothing, and no index or level goes with it here")
_m(W, "dist < bestDist1R)", "dist <= bestDist1R)", "the last of equal best distances wins (right)")
_m(W, "bestDist1 <= TH_LOW", "bestDist1 < TH_LOW", "a best distance of exactly TH_LOW refused (left)")
_m(W, "(float)bestDist1 < nnRatio * (float)bestDist2", "(float)bestDist1 <= nnRatio * (float)bestDist2", "ratio test accepts equality")
_m(W, "bestDist1R <= TH_LOW", "bestDist1R < TH_LOW", "a best distance of exactly TH_LOW refused (right)")
_m(W, "float rot = kfAngle[realIdxKF] - fAngle[bestIdxF];\n                        if (rot < 0.0)", "float rot = kfAngle[realIdxKF] - fAngle[bestIdxF];\n                        if (rot <= 0.0)",
   "a rotation difference of exactly 0 wrapped to 360 (left)")
_m(W, "fAngle[bestIdxF];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)roundf(rot * factor);",
   "fAngle[bestIdxF];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)floorf(rot * factor);", "histogram bin by truncation (left)")
_m(W, "fAngle[bestIdxF];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)roundf(rot * factor);\n                        if (bin == HISTO_LENGTH) bin = 0;",
   "fAngle[bestIdxF];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)roundf(rot * factor);\n                        if (bin == HISTO_LENGTH) bin = HISTO_LENGTH - 1;",
   "bin 30 folded onto bin 29 instead of bin 0 (left)")
_m(W, "fAngle[bestIdxF];\n                        if (rot < 0.0) rot += 360.0f;", "fAngle[bestIdxF];\n                        if (rot < 0.0) rot = -rot;", "negative differences mirrored instead of wrapped (left)")
_m(W, "fAngle[bestIdxFR];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)roundf(rot * factor);",
   "fAngle[bestIdxFR];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)floorf(rot * factor);", "histogram bin by truncation (right)")
_m(W, "float rot = kfAngle[realIdxKF] - fAngle[bestIdxFR];\n                        if (rot < 0.0)", "float rot = kfAngle[realIdxKF] - fAngle[bestIdxFR];\n                        if (rot <= 0.0)",
   "a rotation difference of exactly 0 wrapped to 360 (right)")
_m(W, "fAngle[bestIdxFR];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)roundf(rot * factor);\n                        if (bin == HISTO_LENGTH) bin = 0;",
   "fAngle[bestIdxFR];\n                        if (rot < 0.0) rot += 360.0f;\n                        int bin = (int)roundf(rot * factor);\n                        if (bin == HISTO_LENGTH) bin = HISTO_LENGTH - 1;",
   "bin 30 folded onto bin 29 instead of bin 0 (right)")
_m(W, "fAngle[bestIdxFR];\n                        if (rot < 0.0) rot += 360.0f;", "fAngle[bestIdxFR];\n                        if (rot < 0.0) rot = -rot;", "negative differences mirrored instead of wrapped (right)")
_m(W, "matchOut[bestIdxFR] = realIdxKF;", "matchOut[bestIdxFR] = realIdxKF; if (0)", "right matches left out of the histogram")
_m(W, "if (i == ind1 || i == ind2 || i == ind3) continue;", "if (i == ind1 || i == ind2) continue;", "only two bins kept")

# ---- Frame::isInFrustum ------------------------------------------------------------------------------------------------
I = "orc_is_in_frustum"
_m(I, "p->skip || p->bad", "p->bad", "skipped points projected")
_m(I, "p->skip || p->bad", "p->skip", "bad points projected")
_m(I, "if (pcz < 0.0f) continue; /* :288 */", "", "points behind the camera projected")
_m(I, "u < F->minX", "u <= F->minX", "a projection exactly on minX refused")
_m(I, "u > F->maxX", "u >= F->maxX", "a projection exactly on maxX refused (the bound is closed here)")
_m(I, "v < F->minY", "v <= F->minY", "a projection exactly on minY refused")
_m(I, "v > F->maxY", "v >= F->maxY", "a projection exactly on maxY refused")
_m(I, "if (u < F->minX || u > F->maxX) continue;", "", "horizontal image gate deleted")
_m(I, "if (v < F->minY || v > F->maxY) continue;", "", "vertical image gate deleted")
_m(I, "dist < minD", "dist <= minD", "a distance of exactly 0.9f * minDistance refused")
_m(I, "dist > maxD", "dist >= maxD", "a distance of exactly 1.1f * maxDistance refused")
_m(I, "if (dist < minD || dist > maxD) continue;", "", "distance gate deleted")
_m(I, "1.1f * p->maxDistance", "(float)(1.1 * p->maxDistance)", "1.1 as a double constant")
_m(I, "0.9f * p->minDistance", "(float)(0.9 * p->minDistance)", "0.9 as a double constant")
_m(I, "nScale = (int)ceilf(q);", "nScale = (int)floorf(q) + 1;", "ceil written as floor + 1")
_m(I, "nScale = (int)ceilf(q);", "nScale = (int)roundf(q);", "level by rounding")
_m(I, "if (nScale >= F->nLevels) nScale", "if (nScale > F->nLevels) nScale", "level nLevels not clamped")
_m(I, "q >= (float)F->nLevels) nScale = F->nLevels - 1;", "q >= (float)F->nLevels) nScale = F->nLevels;", "level nLevels for q >= nLevels")
_m(I, "q >= (float)F->nLevels) nScale", "q > (float)F->nLevels) nScale", "q == nLevels sent down the ceil path",
   equivalent="q == nLevels gives ceilf(q) == nLevels, which the clamp inside the ceil path turns into nLevels - 1 as well")
_m(I, "!(q > 0.0f)", "!(q >= 0.0f)", "q == 0 sent down the ceil path", equivalent="q == 0 gives level 0 either way: ceilf(0) is 0")
_m(I, "o->projX = u; /* :299-300", "if (0) o->projX = u; /* :299-300", "projection written only for points in view")

# ---- MapPoint::PredictScale as SearchBySim3 and the relocalisation search call it --------------------------------------
S = "predict_scale"
_m(S, "lvl = (int)ceilf(q);", "lvl = (int)floorf(q) + 1;", "ceil written as floor + 1")
_m(S, "lvl = (int)ceilf(q);", "lvl = (int)roundf(q);", "level by rounding")
_m(S, "if (lvl >= nLevels) lvl", "if (lvl > nLevels) lvl", "level nLevels not clamped")
_m(S, "q >= (float)nLevels", "q > (float)nLevels", "q == nLevels sent down the ceil path",
   equivalent="q == nLevels gives ceilf(q) == nLevels, which the clamp inside the ceil path turns into nLevels - 1 as well")
_m(S, "!(q > 0.0f)", "!(q >= 0.0f)", "q == 0 sent down the ceil path", equivalent="q == 0 gives level 0 either way: ceilf(0) is 0")

# ---- ORBmatcher::SearchBySim3 --------------------------------------------------------------------------------------------
D = "sim3_direction"
_m(D, "p->skip || p->bad", "p->bad", "features without a map point or already matched searched")
_m(D, "p->skip || p->bad", "p->skip", "bad points searched")
_m(D, "if (bz < 0.0f) continue; /* :1032 */", "", "points behind the camera projected")
_m(D, "bz < 0.0f", "bz <= 0.0f", "depth 0 refused before the projection",
   equivalent="at depth 0 invz is infinite, x and y are infinite or NaN (0 * inf), and both fail IsInImage on the next gate")
_m(D, "u >= D->minX", "u > D->minX", "a projection exactly on minX refused")
_m(D, "u < D->maxX", "u <= D->maxX", "a projection exactly on maxX accepted")
_m(D, "v >= D->minY", "v > D->minY", "a projection exactly on minY refused")
_m(D, "v < D->maxY", "v <= D->maxY", "a projection exactly on maxY accepted")
_m(D, "if (!(u >= D->minX && u < D->maxX && v >= D->minY && v < D->maxY)) continue;", "", "image-bounds gate deleted")
_m(D, "dist3D < minD", "dist3D <= minD", "a distance of exactly 0.9f * minDistance refused")
_m(D, "dist3D > maxD", "dist3D >= maxD", "a distance of exactly 1.1f * maxDistance refused")
_m(D, "if (dist3D < minD || dist3D > maxD) continue;", "", "distance gate deleted")
_m(D, "oct < lvl - 1", "oct <= lvl - 1", "level lvl - 1 excluded")
_m(D, "oct < lvl - 1", "oct < lvl - 2", "level lvl - 2 included")
_m(D, "oct > lvl)", "oct >= lvl)", "level lvl excluded")
_m(D, "oct > lvl)", "oct > lvl + 1)", "level lvl + 1 included")
_m(D, "if (oct < lvl - 1 || oct > lvl) continue;", "", "level gate deleted")
_m(D, "dist < bestDist)", "dist <= bestDist)", "the last of equal distances wins")
_m(D, "bestDist <= TH_HIGH", "bestDist < TH_HIGH", "a best distance of exactly TH_HIGH refused")
_m("orc_search_by_sim3", "idx2 >= 0 &&", "idx2 > 0 &&", "a match with feature 0 of key frame 2 lost")
_m("orc_search_by_sim3", "vn2[idx2] == i1", "vn2[idx2] >= 0", "agreement not checked: any match back counts")

# ---- ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, ...) (relocalisation) ----------------------------------
K = "orc_search_by_projection_kf"
_m(K, "p->skip || p->bad", "p->bad", "features without a map point or already found searched")
_m(K, "p->skip || p->bad", "p->skip", "bad points searched")
_m(K, "u < Fr->minX", "u <= Fr->minX", "a projection exactly on minX refused")
_m(K, "u > Fr->maxX", "u >= Fr->maxX", "a projection exactly on maxX refused (closed bound)")
_m(K, "v < Fr->minY", "v <= Fr->minY", "a projection exactly on minY refused")
_m(K, "v > Fr->maxY", "v >= Fr->maxY", "a projection exactly on maxY refused (closed bound)")
_m(K, "if (u < Fr->minX || u > Fr->maxX) continue;", "", "horizontal image gate deleted")
_m(K, "if (v < Fr->minY || v > Fr->maxY) continue;", "", "vertical image gate deleted")
_m(K, "dist3D < minD", "dist3D <= minD", "a distance of exactly 0.9f * minDistance refused")
_m(K, "dist3D > maxD", "dist3D >= maxD", "a distance of exactly 1.1f * maxDistance refused")
_m(K, "if (dist3D < minD || dist3D > maxD) continue;", "", "distance gate deleted")
_m(K, "lvl - 1, lvl + 1, vIndices", "lvl, lvl + 1, vIndices", "level range without lvl - 1")
_m(K, "lvl - 1, lvl + 1, vIndices", "lvl - 1, lvl, vIndices", "level range without lvl + 1")
_m(K, "lvl - 1, lvl + 1, vIndices", "lvl - 2, lvl + 1, vIndices", "level range widened to lvl - 2")
_m(K, "lvl - 1, lvl + 1, vIndices", "lvl - 1, lvl + 2, vIndices", "level range widened to lvl + 2")
_m(K, "if (taken[i2]) continue;", "", "keypoints that hold a map point compete")
_m(K, "taken[bestIdx2] = 1;", "", "a matched keypoint stays free for later points")
_m(K, "dist < bestDist)", "dist <= bestDist)", "the last of equal distances wins")
_m(K, "bestDist <= TH_HIGH", "bestDist < TH_HIGH", "a best distance of exactly TH_HIGH refused")
_m(K, "if (rot < 0.0)", "if (rot <= 0.0)", "a rotation difference of exactly 0 wrapped to 360")
_m(K, "roundf(rot * factor)", "floorf(rot * factor)", "histogram bin by truncation")
_m(K, "if (bin == HISTO_LENGTH) bin = 0;", "if (bin == HISTO_LENGTH) bin = HISTO_LENGTH - 1;", "bin 30 folded onto bin 29 instead of bin 0")

# ---- ORBmatcher::SearchForInitialization -----------------------------------------------------------------------------------
N = "orc_search_for_initialization"
_m(N, "if (level1 > 0) continue;", "", "frame-1 keypoints above level 0 searched")
_m(N, "vMatchedDistance[i2] <= dist", "vMatchedDistance[i2] < dist", "a frame-2 keypoint matched at the same distance competes again")
_m(N, "if (vMatchedDistance[i2] <= dist) continue;", "", "frame-2 keypoints matched at a smaller distance compete again")
_m(N, "dist < bestDist)", "dist <= bestDist)", "the last of equal best distances wins")
_m(N, "dist < bestDist2)", "dist <= bestDist2)", "second best replaced by an equal distance",
   equivalent="bestDist2 is only a value: replacing it by an equal value changes nothing, and no index or level goes with it here")
_m(N, "bestDist <= TH_LOW", "bestDist < TH_LOW", "a best distance of exactly TH_LOW refused")
_m(N, "(float)bestDist < (float)bestDist2 * nnRatio", "(float)bestDist <= (float)bestDist2 * nnRatio", "ratio test accepts equality")
_m(N, "vnMatches21[bestIdx2] >= 0", "vnMatches21[bestIdx2] > 0", "a match of frame-1 keypoint 0 is not withdrawn when it is stolen")
_m(N, "matches12Out[vnMatches21[bestIdx2]] = -1;", "", "the former owner keeps its entry")
_m(N, "vMatchedDistance[bestIdx2] = bestDist;", "", "the distance of a match is not remembered")
_m(N, "if (rot < 0.0)", "if (rot <= 0.0)", "a rotation difference of exactly 0 wrapped to 360")
_m(N, "roundf(rot * factor)", "floorf(rot * factor)", "histogram bin by truncation")
_m(N, "if (bin == HISTO_LENGTH) bin = 0;", "if (bin == HISTO_LENGTH) bin = HISTO_LENGTH - 1;", "bin 30 folded onto bin 29 instead of bin 0")
_m(N, "if (matches12Out[idx1] >= 0) {", "if (1) {", "a withdrawn match deleted (and counted) again by the histogram")

# ---- ORBmatcher::SearchForTriangulation: its own gates (the KannalaBrandt8 epipolar arithmetic is S10 numerics, covered elsewhere) ----
R = "orc_search_for_triangulation_cam"
_m(R, "if (hasMP1[idx1]) continue;", "", "key-frame-1 features with a map point searched")
_m(R, "if (hasMP2[idx2]) continue;", "", "key-frame-2 features with a map point compete")
_m(R, "if (bOnlyStereo && !bStereo1) continue;", "", "bOnlyStereo ignored for key frame 1")
_m(R, "if (bOnlyStereo && !bStereo2) continue;", "", "bOnlyStereo ignored for key frame 2")
_m(R, "dist > TH_LOW ||", "dist >= TH_LOW ||", "a distance of exactly TH_LOW refused")
_m(R, "dist > bestDist)", "dist >= bestDist)", "the earlier of equal distances wins (the reference lets the later one replace it)")
_m(R, "!bStereo1 && !bStereo2 && !noEpipoleGate", "!bStereo2 && !noEpipoleGate", "epipole gate applied although key frame 1's keypoint is stereo")
_m(R, "!bStereo1 && !bStereo2 && !noEpipoleGate", "!bStereo1 && !noEpipoleGate", "epipole gate applied although key frame 2's keypoint is stereo")
_m(R, "err < 100 * scaleFactors2", "err <= 100 * scaleFactors2", "a keypoint exactly 100 * sf from the epipole dropped")
_m(R, "if (err < 100 * scaleFactors2[k2->octave]) continue;", "", "epipole gate deleted")
_m(R, "scaleFactors2[k2->octave]", "scaleFactors2[k1->octave]", "epipole gate scaled by key frame 1's level")
_m(R, "ok = dsqr < 3.84 * 1.0;", "ok = 1;", "epipolar gate deleted")
_m(R, "dsqr < 3.84 * 1.0", "dsqr < 3.84f", "epipolar gate against the float constant: 3.84f itself, which lies below 3.84, is refused")
_m(R, "dsqr < 3.84 * 1.0", "dsqr <= 3.84 * 1.0", "epipolar gate accepts equality",
   equivalent="dsqr is a binary32 number and 3.84 is not one, so equality with the double constant cannot occur")
_m(R, "if (bestIdx2 >= 0) {", "if (bestIdx2 > 0) {", "a match with feature 0 of key frame 2 lost")
_m(R, "bestDist = dist;", "", "the bar is not lowered by an accepted candidate")
_m(R, "if (rot < 0.0)", "if (rot <= 0.0)", "a rotation difference of exactly 0 wrapped to 360")
_m(R, "roundf(rot * factor)", "floorf(rot * factor)", "histogram bin by truncation")
_m(R, "if (bin == HISTO_LENGTH) bin = 0;", "if (bin == HISTO_LENGTH) bin = HISTO_LENGTH - 1;", "bin 30 folded onto bin 29 instead of bin 0")

MUTANTS = M


def function_span(text, name):
    """(start, end) of the body of function `name` in `text`, braces included"""
    m = re.search(r"^[A-Za-z][^\n;{}()]*\b%s\s*\([^;{}]*\)\s*\{" % re.escape(name), text, re.M)
    if not m:
        raise ValueError("function %s not found in the oracle" % name)
    depth, i = 0, m.end() - 1
    while True:
        depth += text[i] == "{"
        depth -= text[i] == "}"
        if depth == 0:
            return m.start(), i + 1
        i += 1


def mutate(text, mutant):
    a, b = function_span(text, mutant["fn"])
    n = text[a:b].count(mutant["anchor"])
    if n != 1:
        raise ValueError("mutant %s: anchor %r occurs %d times in %s (must be exactly once)" % (mutant["id"], mutant["anchor"], n, mutant["fn"]))
    return text[:a] + text[a:b].replace(mutant["anchor"], mutant["repl"]) + text[b:]


def _cflags():
    with open(os.path.join(O.ODIR, "Makefile")) as f:
        line = next(l for l in f if l.startswith("CFLAGS"))
    return line.split("=", 1)[1].split() + ["-O1", "-g0", "-w"]


class Builder:
    """Builds mutants (and the unmutated control) of the oracle in a temporary directory outside the tree."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="gate_mutants_")
        atexit.register(self.close)
        self.cc = os.environ.get("CC", "gcc")
        self.flags = _cflags()
        with open(SOURCE) as f:
            self.text = f.read()
        self.objs = []
        for src in OTHERS:  # the two other sources are the same for every mutant: compiled once
            obj = os.path.join(self.dir, src[:-2] + ".o")
            subprocess.check_call([self.cc] + self.flags + ["-c", "-o", obj, os.path.join(O.ODIR, src)])
            self.objs.append(obj)

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def _build(self, tag, text):
        d = os.path.join(self.dir, tag)
        os.makedirs(d)
        src, so = os.path.join(d, "match_oracle.c"), os.path.join(d, "liborb_oracle_%s.so" % tag)
        with open(src, "w") as f:
            f.write(text)
        subprocess.check_call([self.cc] + self.flags + ["-I", O.ODIR, "-shared", "-o", so, src] + self.objs + ["-lm"])
        return so

    def control(self):
        return O.bind(self._build("control", self.text))

    def build_all(self, mutants):
        """{mutant id: bound library}; a missing or ambiguous anchor raises before anything is compiled"""
        texts = [(re.sub(r"\W", "_", m["id"]), mutate(self.text, m)) for m in mutants]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_JOBS, os.cpu_count() or 1)) as ex:
            paths = list(ex.map(lambda t: self._build(*t), texts))
        return {m["id"]: O.bind(p) for m, p in zip(mutants, paths)}
