"""The ABI of the two S23 calls (orbfe_track_inertial_batch_device, orbfe_track_frame_inertial): the symbols, the blocks against the
header's figures, and the refusals that the arguments alone decide -- struct sizes outer and nested, required NULLs, batch < 1,
n_points < 0, descending sample offsets, a missing prior for the last-frame kind, the branches that are not built -- which come back
before a handle or a device is looked at (the handle is NULL throughout)."""
import ctypes as C

import numpy as np

INVALID, UNSUPPORTED = 1, 2
NAMES = ("orbfe_track_inertial_batch_device", "orbfe_track_frame_inertial")


def test_symbols_exported(built):
    import orbfe
    L = orbfe.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in orbfe.SYMBOLS


def test_blocks_match_the_header(built):
    import orbfe
    P = orbfe.TrackInertialParams
    # struct_size, inlier_threshold, then the nested blocks in the header's order; the two pose blocks hold doubles: 8-byte aligned
    sizes = dict(track=44, noise=56, predict=72, frustum=124, pose_keyframe=104, pose_frame=120)
    at = 8
    for name in ("track", "noise", "predict", "frustum", "pose_keyframe", "pose_frame"):
        f = getattr(P, name)
        at = (at + 7) // 8 * 8 if name.startswith("pose") else at
        assert (f.offset, f.size) == (at, sizes[name]), (name, f.offset, f.size)
        at += sizes[name]
    assert P().struct_size == C.sizeof(P) == at == 528 and P.inlier_threshold.offset == 4 and P().inlier_threshold == 8
    p = P()
    assert p.track.struct_size == 44 and p.noise.struct_size == 56 and p.predict.struct_size == 72
    assert p.pose_keyframe.struct_size == 104 and p.pose_frame.struct_size == 120 and p.pose_frame.inlier_threshold == 8
    IO = orbfe.TrackInertialIO
    assert IO().struct_size == C.sizeof(IO) == 8 + 8 * len(orbfe.TRACK_INERTIAL_IO_FIELDS) == 240
    assert (IO.d_samples.offset, IO.sample_off.offset, IO.d_kp.offset, IO.d_state_in.offset, IO.d_Tcw_out.offset) == (8, 16, 80, 120, 232)
    R = orbfe.TrackInertialResult
    assert R().struct_size == C.sizeof(R) == 160 and (R.steps_out.offset, R.info_ok.offset, R.mp_out.offset, R.n_inliers.offset,
                                                      R.Tcw.offset) == (8, 32, 40, 96, 112)


def _good(orbfe, which=0):
    p = orbfe.TrackInertialParams(predict=orbfe.ImuPredictParams(which))
    p.track.grid_cols, p.track.grid_rows, p.track.grid_inv_w, p.track.grid_inv_h = 64, 48, 0.1, 0.1
    p.frustum.n_levels, p.frustum.log_scale_factor = 8, 0.18
    return p


def test_argument_errors_without_a_device(built):
    import orbfe
    L = orbfe.lib()
    N, B = None, C.byref
    one = 4096   # a non-NULL stand-in for device pointers and the map: the call is refused before any of them is read
    good_off = np.array([0, 3, 3, 8], np.int32)

    def io_of(off=good_off, which=0, **over):
        k = {name: one for name in orbfe.TRACK_INERTIAL_IO_FIELDS}
        k["sample_off"] = off.ctypes.data if off is not None else None
        k["d_steps_out"] = k["d_Hprior_out"] = None
        if which == 0:
            k["d_priors"] = None
        k.update(over)
        return orbfe.TrackInertialIO(**k)

    def bat(p=None, batch=3, kp_stride=200, map_=one, M=70, io=None, which=0):
        p = _good(orbfe, which) if p is None else p
        io = io_of(which=which) if io is None else io
        return L.orbfe_track_inertial_batch_device(N, B(p) if p else N, batch, kp_stride, map_, M, B(io) if io else N, N)

    # every argument in order, a NULL handle: INVALID_ARG at the end of the ladder, and only there
    assert bat() == INVALID and bat(which=1) == INVALID
    assert bat(p=False) == INVALID and bat(io=False) == INVALID

    def wrong(edit, which=0):
        p = _good(orbfe, which)
        edit(p)
        return p

    def size(name):
        def f(p):
            blk = p if name is None else getattr(p, name)
            blk.struct_size -= 4
        return f
    for name in (None, "track", "noise", "predict", "pose_keyframe"):
        assert bat(p=wrong(size(name))) == INVALID, name
    assert bat(p=wrong(size("pose_frame"), 1), which=1) == INVALID
    assert bat(p=wrong(size("pose_frame"), 0)) == INVALID          # NULL handle; the unused pose block is not what refuses it:
    pk = wrong(size("pose_frame"), 0)
    pk.pose_keyframe.camera_model = 1                              # ... the block in use is read, the other is not
    assert bat(p=pk) == UNSUPPORTED
    io = io_of()
    io.struct_size -= 8
    assert bat(io=io) == INVALID
    assert bat(p=wrong(lambda p: setattr(p.predict, "which", 2))) == INVALID
    # the branches that are not built: KannalaBrandt8 in the frustum template or the pose block, stereo
    assert bat(p=wrong(lambda p: setattr(p.frustum, "camera_model", 1))) == UNSUPPORTED
    assert bat(p=wrong(lambda p: setattr(p.pose_keyframe, "camera_model", 1))) == UNSUPPORTED
    assert bat(p=wrong(lambda p: setattr(p.pose_keyframe, "stereo", 1))) == UNSUPPORTED
    assert bat(p=wrong(lambda p: setattr(p.pose_frame, "stereo", 1), 1), which=1) == UNSUPPORTED
    assert bat(p=wrong(lambda p: setattr(p.pose_frame, "camera_model", 1), 1), which=1) == UNSUPPORTED
    assert bat(p=wrong(lambda p: setattr(p.frustum, "n_levels", 0))) == INVALID
    assert bat(p=wrong(lambda p: setattr(p.track, "grid_cols", 0))) == INVALID
    # counts and offsets
    assert bat(batch=0) == INVALID and bat(M=-1) == INVALID and bat(kp_stride=0) == INVALID and bat(kp_stride=65537) == INVALID
    assert bat(map_=N) == INVALID
    assert bat(io=io_of(off=None)) == INVALID and bat(io=io_of(off=np.array([0, 5, 3, 8], np.int32))) == INVALID
    assert bat(io=io_of(off=np.array([-1, 3, 3, 8], np.int32))) == INVALID
    # every required pointer; the optional ones (d_steps_out, d_Hprior_out; d_priors for the key-frame kind) were NULL above
    optional = {"d_steps_out", "d_Hprior_out", "d_priors", "sample_off"}
    seen = []
    for name in orbfe.TRACK_INERTIAL_IO_FIELDS:
        if name in optional:
            continue
        assert bat(io=io_of(**{name: None})) == INVALID, name
        seen.append(name)
    assert len(seen) == len(orbfe.TRACK_INERTIAL_IO_FIELDS) - 4
    assert bat(io=io_of(which=1, d_priors=None), which=1) == INVALID   # the last-frame kind needs its prior
    # M == 0 needs neither ids, records nor found flags: what is left to refuse is the NULL handle
    assert bat(M=0, io=io_of(d_ids=None, d_mp_out=None, d_found=None)) == INVALID

    # ---- the single-frame call ----
    smp = np.zeros(4, orbfe.IMU_SAMPLE_DTYPE)
    bias, s1 = np.zeros(6, np.float32), np.zeros(21, np.float32)
    kf, fr, prior = orbfe.ImuPreint(), orbfe.ImuPreint(), orbfe.PoseImuPrior()
    n = C.c_int(7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def res_of(**over):
        k = dict(steps_out=None, state_in=one, link_out=None, mp_out=one, match_out=one, state_out=one, H_out=one, Hprior_out=None,
                 outlier=one, found=one)
        k.update(over)
        return orbfe.TrackInertialResult(**k)

    def one_frame(p=None, which=0, gray=one, ns=4, smp_=ptr(smp), bias_=ptr(bias), s1_=ptr(s1), kf_=kf, fr_=fr, map_=one, M=70, ids=one,
                  prior_=None, kp=one, desc=one, n_=B(n), res=None):
        p = _good(orbfe, which) if p is None else p
        res = res_of() if res is None else res
        return L.orbfe_track_frame_inertial(N, B(p) if p else N, gray, 752, ns, smp_, 1.0, 2.0, bias_, s1_, B(kf_) if kf_ else N,
                                            B(fr_) if fr_ else N, map_, M, ids, B(prior_) if prior_ else N, kp, desc, n_, N,
                                            B(res) if res else N)
    assert one_frame() == INVALID and one_frame(which=1, prior_=prior) == INVALID
    assert one_frame(p=False) == INVALID and one_frame(res=False) == INVALID
    assert one_frame(p=wrong(size(None))) == INVALID and one_frame(p=wrong(size("track"))) == INVALID
    bad_rec = orbfe.ImuPreint()
    bad_rec.struct_size -= 4
    assert one_frame(kf_=bad_rec) == INVALID and one_frame(fr_=bad_rec) == INVALID
    r = res_of()
    r.struct_size -= 4
    assert one_frame(res=r) == INVALID
    assert one_frame(p=wrong(lambda p: setattr(p.frustum, "camera_model", 1))) == UNSUPPORTED
    assert one_frame(p=wrong(lambda p: setattr(p.pose_keyframe, "stereo", 1))) == UNSUPPORTED
    assert one_frame(gray=N) == INVALID and one_frame(ns=-1) == INVALID and one_frame(smp_=N) == INVALID and one_frame(bias_=N) == INVALID
    assert one_frame(s1_=N) == INVALID and one_frame(kf_=False) == INVALID and one_frame(fr_=False) == INVALID and one_frame(map_=N) == INVALID
    assert one_frame(M=-1) == INVALID and one_frame(ids=N) == INVALID and one_frame(kp=N) == INVALID and one_frame(desc=N) == INVALID
    assert one_frame(n_=N) == INVALID and one_frame(which=1) == INVALID      # the last-frame kind without a prior
    for name in ("state_in", "mp_out", "match_out", "state_out", "H_out", "outlier", "found"):
        assert one_frame(res=res_of(**{name: None})) == INVALID, name
    assert n.value == 7
