// Monotone path through a score matrix (attn_probs.h): the text-to-audio alignment's decoding step.
//
//   dp[0][i] = score[0][i];   dp[j][i] = score[j][i] + max_{i' <= i} dp[j-1][i']
//
// One workgroup per sample, thread i owns column i and keeps dp[j][i] in a register.  Per row: an inclusive prefix (max, argmax) scan
// over the columns - shuffles inside a wave, the wave totals through LDS - under the operator "the later element wins only when strictly
// larger", which is associative and yields the LOWEST index among equal maxima; then one fp32 add.  Back-pointers go to global memory as
// int16; the path ends at the lowest argmax of the last row and thread 0 walks it back.  Every cell is one add and compares: the result
// is that of the same recurrence in any other fp32 implementation, bit for bit.
#include "attn_probs.h"
#include "prof.h"

namespace dtts {

__global__ __launch_bounds__(1024) void monotone_path_kernel(const float* __restrict__ score, const int* __restrict__ n_, const int* __restrict__ m_,
                                                             int n_max, int m_max, short* __restrict__ back, int* __restrict__ path) {
    __shared__ float wv[2][16];
    __shared__ int wi[2][16];
    __shared__ int end_i;
    const int b = blockIdx.x, i = threadIdx.x, lane = i & 63, wave = i >> 6;
    const int n = n_[b], m = m_[b];
    int* pb = path + (long long)b * n_max;
    for (int jj = i; jj < n_max; jj += blockDim.x)
        if (jj >= n) pb[jj] = -1;
    if (n <= 0 || m <= 0) return;                       // workgroup-uniform
    const float* sb = score + (long long)b * n_max * m_max;
    short* bb = back + (long long)b * n_max * m_max;
    const bool live = i < m;

    float dp = live ? sb[i] : -INFINITY;
    float nxt = (live && n > 1) ? sb[m_max + i] : 0.f;   // row j + 1 is fetched while row j is scanned
    for (int jrow = 1; jrow <= n; ++jrow) {
        // inclusive prefix (max, lowest argmax) of the previous row's dp; after row n - 1 once more, for the path's end
        float v = dp;
        int a = i;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float ov = __shfl_up(v, d);
            const int oa = __shfl_up(a, d);
            if (lane >= d && !(v > ov)) { v = ov; a = oa; }
        }
        const int buf = jrow & 1;
        if (lane == 63) { wv[buf][wave] = v; wi[buf][wave] = a; }
        __syncthreads();
        if (wave > 0) {
            float pv = wv[buf][0];
            int pa = wi[buf][0];
            for (int w = 1; w < wave; ++w)
                if (wv[buf][w] > pv) { pv = wv[buf][w]; pa = wi[buf][w]; }
            if (!(v > pv)) { v = pv; a = pa; }
        }
        if (jrow == n) {
            if (i == m - 1) end_i = a;
            break;
        }
        const float sc = nxt;
        if (live && jrow + 1 < n) nxt = sb[(long long)(jrow + 1) * m_max + i];
        if (live) {
            dp = sc + v;
            bb[(long long)jrow * m_max + i] = (short)a;
        }
    }
    __syncthreads();            // back-pointers and end_i are visible to thread 0
    if (i == 0) {
        int c = end_i;
        for (int jrow = n - 1; jrow >= 0; --jrow) {
            pb[jrow] = c;
            if (jrow > 0) c = bb[(long long)jrow * m_max + c];
        }
    }
}

void launch_monotone_path(const float* score, const int* n, const int* m, int B, int n_max, int m_max, short* back, int* path,
                          hipStream_t stream) {
    DTTS_REQUIRE(B > 0 && n_max > 0 && m_max > 0 && m_max <= ALIGN_PATH_MAX_M, "monotone path: sizes");
    DTTS_REQUIRE(score && n && m && back && path, "monotone path: null argument");
    ProfScope ps("monotone_path_kernel", 0.0, 6.0 * B * (double)n_max * m_max, stream);
    hipLaunchKernelGGL(monotone_path_kernel, dim3(B), dim3(round_up(m_max, 64)), 0, stream, score, n, m, n_max, m_max, back, path);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
