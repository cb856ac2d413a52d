// kernels_distinct.hip -- MapPoint::ComputeDistinctiveDescriptors for a batch of map points (SURVEY.md section 8f,
// honourable mention): the N x N Hamming-median selection of src/MapPoint.cc:343-416.
//
// One thread per (set, row i): the median of row i is its k-th smallest distance, k = (size_t)(0.5 * (N - 1)), row
// including the zero self-distance.  Distances lie in 0..256, so the k-th smallest is found by a 9-step binary
// search over the VALUE (count of distances <= v, recomputing the popcounts from L2-resident descriptors) instead
// of materialising and sorting the row; the representative = min over rows of (median << 20 | i) by one atomicMin
// per row -- the first minimum wins, as the strict "<" of the reference (:403).  Sets are small (observations of
// one map point), the batch supplies the parallelism.
#include <algorithm>
#include <cstring>

#include "distinct_select.h"
#include "match_common.h"

namespace orbfe {

namespace {

__global__ __launch_bounds__(256) void distinct_kernel(int nRows, const int* __restrict__ rowSet, const int* __restrict__ setOff,
                                                       const uint8_t* __restrict__ desc, unsigned int* __restrict__ best)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nRows) return;
    const int s = rowSet[r];
    const int lo = setOff[s], hi = setOff[s + 1];
    const int N = hi - lo, i = r - lo;
    const int k = distinct_median_position(N);
    unsigned long long d4[4];
    const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(desc + (size_t)r * 32);
    d4[0] = dp[0]; d4[1] = dp[1]; d4[2] = dp[2]; d4[3] = dp[3];
    const int median = distinct_kth_distance(k, [&](int v) {   // recomputing the popcounts from L2-resident descriptors
        int c = 0;
        for (int j = lo; j < hi; j++) {
            const int dist = j == r ? 0 : hamming256(reinterpret_cast<const uint2*>(desc + (size_t)j * 32), d4);
            c += dist <= v;
        }
        return c;
    });
    atomicMin(&best[s], distinct_pack(median, i));
}

}  // namespace

int distinctive_run(MatchScratch& m, hipStream_t s, int nSets, const int* setOff, const uint8_t* desc, int* bestIdx,
                    int* bestMedian, std::string& err)
{
    if (nSets == 0) return ORBFE_OK;
    const int nRows = setOff[nSets];
    for (int q = 0; q < nSets; q++) {
        const int n = setOff[q + 1] - setOff[q];
        if (n < 0 || n >= (1 << kDistinctIndexBits)) return ORBFE_ERR_INVALID_ARG;
        bestIdx[q] = -1;
        if (bestMedian) bestMedian[q] = 0;
    }
    if (nRows == 0) return ORBFE_OK;
    Staging st;
    const auto bOff = st.in<int>((size_t)nSets + 1);
    const auto bRowSet = st.in<int>(nRows);
    const auto bDesc = st.in<uint8_t>((size_t)nRows * 32);
    const auto bBest = st.inout<unsigned int>(nSets);   // goes up as "none", comes down as the packed minimum
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bOff, setOff);
    int* rowSet = st.host(bRowSet);
    for (int q = 0; q < nSets; q++)
        for (int r = setOff[q]; r < setOff[q + 1]; r++) rowSet[r] = q;
    st.put(bDesc, desc);
    memset(st.host(bBest), 0xff, bBest.bytes());
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    hipLaunchKernelGGL(distinct_kernel, dim3((nRows + 255) / 256), dim3(256), 0, s, nRows, st.dev(bRowSet), st.dev(bOff), st.dev(bDesc),
                       st.dev(bBest));
    if ((rc = download_span(st, s, bBest.off, bBest.end(), err)) != ORBFE_OK) return rc;
    const unsigned int* hBest = st.res(bBest);
    for (int q = 0; q < nSets; q++)
        if (setOff[q + 1] > setOff[q]) {
            bestIdx[q] = (int)(hBest[q] & ((1u << kDistinctIndexBits) - 1));
            if (bestMedian) bestMedian[q] = (int)(hBest[q] >> kDistinctIndexBits);
        }
    return ORBFE_OK;
}

}  // namespace orbfe
