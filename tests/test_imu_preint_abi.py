"""The ABI of the five S22 calls (orbfe_imu_preintegrate_frame, orbfe_imu_reintegrate, orbfe_imu_predict,
orbfe_imu_frame_batch_device, orbfe_imu_reintegrate_batch_device): the symbols, the blocks against the header's figures, and the
refusals that the arguments alone decide -- struct sizes, NULLs, a negative sample count, descending CSR offsets -- which come back
before a handle or a device is looked at."""
import ctypes as C

import numpy as np

import imu_preint_ref as R
import imu_preint_scenarios as PS

INVALID = 1
NAMES = ("orbfe_imu_preintegrate_frame", "orbfe_imu_reintegrate", "orbfe_imu_predict", "orbfe_imu_frame_batch_device",
         "orbfe_imu_reintegrate_batch_device")


def test_symbols_exported(built):
    import orbfe
    L = orbfe.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in orbfe.SYMBOLS


def test_blocks_match_the_header(built):
    import orbfe
    assert orbfe.IMU_SAMPLE_DTYPE.itemsize == 32 and orbfe.IMU_SAMPLE_DTYPE.fields["a"][1] == 8      # sizeof(orbfe_imu_sample) == 32
    assert orbfe.IMU_STEP_DTYPE.itemsize == 32 and orbfe.IMU_STEP_DTYPE.fields["dt"][1] == 24
    assert orbfe.ImuNoise().struct_size == C.sizeof(orbfe.ImuNoise) == 8 + 12 * 4
    P = orbfe.ImuPreint
    assert P().struct_size == C.sizeof(P) == 8 + 298 * 4
    # the record's float block is contiguous from dT to C, in the order of imu_preint_ref.REC_FIELDS
    at = 8
    for name, n in R.REC_FIELDS:
        f = getattr(P, name)
        assert (f.offset, f.size) == (at, 4 * n), name
        at += 4 * n
    assert at == C.sizeof(P) and P.n_steps.offset == 4
    Q = orbfe.ImuPredictParams
    assert Q().struct_size == C.sizeof(Q) == 12 + 15 * 4
    assert (Q.which.offset, Q.gravity.offset, Q.Rcb.offset, Q.tcb.offset, Q.tbc.offset) == (4, 8, 12, 48, 60)
    assert np.float32(Q().gravity) == np.float32(9.81) and (orbfe.IMU_FROM_KEYFRAME, orbfe.IMU_FROM_FRAME) == (0, 1)
    # a record survives the round trip through the block
    sc = PS.make("moving", 3, 0)
    rec = P(sc["kf"].floats(), sc["kf"].n_steps)
    assert rec.floats().tobytes() == sc["kf"].floats().tobytes() and rec.n_steps == 5 and rec.dR[0] == sc["kf"].dR[0, 0]
    assert rec.C[224] == sc["kf"].C[14, 14] > 0


def _wrong(block):
    block.struct_size -= 4
    return block


def test_argument_errors_without_a_device(built):
    """wrong struct_size, NULLs, a negative sample count and descending offsets are INVALID_ARG with a NULL handle: nothing is
    dereferenced and no device is touched"""
    import orbfe
    L = orbfe.lib()
    sc = PS.make("moving", 3, 0)
    noise = orbfe.ImuNoise(sc["noise"].cov, sc["noise"].walk)
    par = orbfe.ImuPredictParams(0, sc["gravity"], sc["Rcb"], sc["tcb"], sc["tbc"])
    smp = np.zeros(4, orbfe.IMU_SAMPLE_DTYPE)
    steps = np.zeros(3, orbfe.IMU_STEP_DTYPE)
    bias, s1, out33 = np.zeros(6, np.float32), np.zeros(21, np.float32), np.zeros(33, np.float32)
    kf, fr, link, n, ok = orbfe.ImuPreint(), orbfe.ImuPreint(), orbfe.ImuLink(), C.c_int(7), C.c_int(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    B, N = C.byref, None

    def pre(noise_=noise, n_=4, smp_=p(smp), bias_=p(bias), kf_=B(kf), fr_=B(fr), nst=B(n)):
        return L.orbfe_imu_preintegrate_frame(N, noise_ and B(noise_), n_, smp_, 1.0, 2.0, bias_, kf_, fr_, N, nst)
    assert pre() == INVALID                                   # no handle
    assert pre(noise_=_wrong(orbfe.ImuNoise())) == INVALID and pre(kf_=B(_wrong(orbfe.ImuPreint()))) == INVALID
    assert pre(fr_=B(_wrong(orbfe.ImuPreint()))) == INVALID
    assert pre(noise_=None) == INVALID and pre(smp_=N) == INVALID and pre(bias_=N) == INVALID and pre(kf_=N) == INVALID
    assert pre(fr_=N) == INVALID and pre(nst=N) == INVALID and pre(n_=-1) == INVALID
    assert n.value == 7

    def rei(noise_=noise, bias_=p(bias), n_=3, st=p(steps), out=B(fr)):
        return L.orbfe_imu_reintegrate(N, noise_ and B(noise_), bias_, n_, st, out)
    assert rei() == INVALID and rei(noise_=_wrong(orbfe.ImuNoise())) == INVALID and rei(noise_=None) == INVALID
    assert rei(bias_=N) == INVALID and rei(n_=-1) == INVALID and rei(st=N) == INVALID and rei(out=N) == INVALID

    def prd(par_=par, s1_=p(s1), kf_=B(kf), fr_=B(fr), out=p(out33), lk=B(link), ok_=B(ok)):
        return L.orbfe_imu_predict(N, par_ and B(par_), s1_, kf_, fr_, out, lk, ok_)
    assert prd() == INVALID and prd(par_=_wrong(orbfe.ImuPredictParams())) == INVALID and prd(par_=orbfe.ImuPredictParams(which=2)) == INVALID
    assert prd(kf_=B(_wrong(orbfe.ImuPreint()))) == INVALID and prd(fr_=B(_wrong(orbfe.ImuPreint()))) == INVALID
    assert prd(par_=None) == INVALID and prd(s1_=N) == INVALID and prd(kf_=N) == INVALID and prd(out=N) == INVALID and prd(lk=N) == INVALID
    assert prd(ok_=N) == INVALID and ok.value == 7

    one = 4096   # a non-NULL stand-in for device pointers: the call is refused before any of them is read
    good = np.array([0, 3, 3, 8], np.int32)

    def bat(noise_=noise, par_=par, batch=3, off=good, ptr=one):
        return L.orbfe_imu_frame_batch_device(N, noise_ and B(noise_), par_ and B(par_), batch, ptr, p(off) if off is not None else N,
                                              *([ptr] * 5), ptr, ptr, N, ptr, ptr, ptr, N)
    assert bat() == INVALID
    assert bat(noise_=_wrong(orbfe.ImuNoise())) == INVALID and bat(par_=_wrong(orbfe.ImuPredictParams())) == INVALID
    assert bat(noise_=None) == INVALID and bat(par_=None) == INVALID and bat(batch=0) == INVALID and bat(off=None) == INVALID
    assert bat(off=np.array([0, 5, 3, 8], np.int32)) == INVALID and bat(off=np.array([-1, 3, 3, 8], np.int32)) == INVALID
    assert bat(ptr=N) == INVALID

    def rbat(noise_=noise, batch=3, off=good, ptr=one):
        return L.orbfe_imu_reintegrate_batch_device(N, noise_ and B(noise_), batch, ptr, p(off) if off is not None else N, ptr, ptr, N)
    assert rbat() == INVALID and rbat(noise_=_wrong(orbfe.ImuNoise())) == INVALID and rbat(noise_=None) == INVALID
    assert rbat(batch=0) == INVALID and rbat(off=None) == INVALID and rbat(off=np.array([0, 5, 3, 8], np.int32)) == INVALID
    assert rbat(ptr=N) == INVALID
