// marginalize.h -- Optimizer::Marginalize(H, 0, 14) (src/Optimizer.cc:2882-2962) of the 30 x 30 Hessian of
// PoseInertialOptimizationLastFrame (SPEC DECISION S20): Hp = Hcc - (Hcb pinv(Hbb)) Hbc with b = rows 0-14, c = rows 15-29.
// Eigen::JacobiSVD is unpinned; for a symmetric matrix V S^+ U^T equals Q L^+ Q^T with the threshold on |lambda|, so the
// pseudo-inverse is pinned as a symmetric Jacobi eigen-decomposition of Hbb (its upper triangle, mirrored): kMargSweeps cyclic sweeps
// in the pair order (0,1) (0,2) .. (13,14), the angle of jacobi.h::jacobi_angle, no data-dependent exit, apq == 0.0 skipped; lambda is
// inverted when |lambda| > 1e-6, else 0.  Every product is a sequential sum in column order, first product first.
// The text is written once over an executor X: X.each(n, f) runs f(t) for t in [0, n) -- one after the other on the host, spread over
// the block and closed by a barrier on the device -- and X.sync() is that barrier alone.  Inside one each() no item reads what another
// item of it writes, so both executions give the same bytes.  Contraction is off in every including unit.
#pragma once
#include <cmath>

#include "host_device.h"
#include "jacobi.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

constexpr int kMargN = 15;
constexpr int kMargLd = 30;                // row stride of the Hessian handed in
constexpr int kMargSweeps = 9;             // S20: fixed on the CPU (DESIGN.md S20 records how), no data-dependent exit
constexpr double kMargThreshold = 1e-6;    // (:2926)

struct MargWork {
    double M[kMargN][kMargN], V[kMargN][kMargN], P[kMargN][kMargN], T[kMargN][kMargN];
};

// one thread after the other: the host form
struct SeqExec {
    template <class F>
    void each(int n, F f)
    {
        for (int t = 0; t < n; t++) f(t);
    }
    void sync() {}
};

template <class Exec>
ORBFE_HD inline void marginalize_run(Exec& X, MargWork& W, const double* H, double* Hp)
{
    constexpr int N = kMargN;
    X.each(N * N, [&](int t) {
        const int i = t / N, j = t % N;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        W.M[i][j] = H[kMargLd * lo + hi];
        W.V[i][j] = i == j ? 1.0 : 0.0;
    });
    for (int sweep = 0; sweep < kMargSweeps; sweep++)
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const double apq = W.M[p][q];
                const bool skip = apq == 0.0;
                double c = 1.0, sn = 0.0;
                if (!skip) jacobi_angle(W.M[p][p], W.M[q][q], apq, c, sn);
                X.sync();   // every reader of M has its angle before a column is rewritten
                if (skip) continue;
                X.each(N, [&](int k) {   // columns p, q of M
                    const double a = W.M[k][p], b = W.M[k][q];
                    W.M[k][p] = c * a - sn * b;
                    W.M[k][q] = sn * a + c * b;
                });
                X.each(N, [&](int k) {   // rows p, q of M; columns p, q of V
                    const double a = W.M[p][k], b = W.M[q][k];
                    W.M[p][k] = c * a - sn * b;
                    W.M[q][k] = sn * a + c * b;
                    const double va = W.V[k][p], vb = W.V[k][q];
                    W.V[k][p] = c * va - sn * vb;
                    W.V[k][q] = sn * va + c * vb;
                });
            }
    X.each(N * N, [&](int t) {   // pinv = (V L^+) V^T
        const int i = t / N, j = t % N;
        double acc = 0.0;
        for (int k = 0; k < N; k++) {
            const double lam = W.M[k][k];
            const double inv = fabs(lam) > kMargThreshold ? 1.0 / lam : 0.0;
            const double term = (W.V[i][k] * inv) * W.V[j][k];
            acc = k == 0 ? term : acc + term;
        }
        W.P[i][j] = acc;
    });
    X.each(N * N, [&](int t) {   // Hcb pinv
        const int i = t / N, j = t % N;
        double acc = 0.0;
        for (int k = 0; k < N; k++) {
            const double term = H[kMargLd * (N + i) + k] * W.P[k][j];
            acc = k == 0 ? term : acc + term;
        }
        W.T[i][j] = acc;
    });
    X.each(N * N, [&](int t) {   // Hcc - (Hcb pinv) Hbc
        const int i = t / N, j = t % N;
        double acc = 0.0;
        for (int k = 0; k < N; k++) {
            const double term = W.T[i][k] * H[kMargLd * k + (N + j)];
            acc = k == 0 ? term : acc + term;
        }
        Hp[N * i + j] = H[kMargLd * (N + i) + (N + j)] - acc;
    });
}

}  // namespace orbfe
