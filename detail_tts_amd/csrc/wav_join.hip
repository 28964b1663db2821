// Long-form synthesis (detail_tts_amd/longform.py): the waveforms of a group of chunks - each a complete utterance, a row of infer's
// padded [B, 1, 1024 n_max] result - are cut at their loud edges and laid end to end with silence between them, on the device.  Two
// kernels that touch waveforms only; the reference has no long-form path, so the yardstick is tests/longform_ref.py.
#include <cmath>

#include "model.h"

namespace dtts {

namespace {

constexpr int EDGE_THREADS = 256;       // 4 waves per row, a frame per wave at a time
constexpr int JOIN_THREADS = 256;       // 4 output samples per thread
constexpr int JOIN_ROWS = 16;          // rows a launch takes: their host tables travel as kernel arguments

struct EdgeLens {
    int len[JOIN_ROWS];
};

// Where a row is loud.  One workgroup per row; wave w takes frames w, w + 4, ...  Lane l of a frame's wave sums the squares of the
// quads l, l + 64, ... of the frame (a quad = 4 consecutive samples, added in ascending order; one 16-byte load where the quad lies
// inside the frame and its address is 16-byte aligned, guarded scalar loads otherwise: the same sum either way), then a butterfly over
// the 64 lanes: a fixed order, the same bits from call to call.  A frame is loud when sum >= thr2 count, count its own sample count
// (the last frame of a row may be partial).  First / last loud frame through LDS integer min / max, which do not depend on the order
// the waves arrive in.  Samples at or beyond len[b] are never loaded.
__global__ __launch_bounds__(EDGE_THREADS) void wav_edges_kernel(const float* __restrict__ wav, EdgeLens lens, int stride, int frame,
                                                                  float thr2, int keep, int* __restrict__ edges) {
    __shared__ int s_first, s_last;
    const int b = blockIdx.x, len = lens.len[b];
    const int nframes = (int)(((long long)len + frame - 1) / frame);
    if (threadIdx.x == 0) { s_first = nframes; s_last = -1; }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row = (size_t)b * stride;
    for (int f = wave; f < nframes; f += EDGE_THREADS / 64) {
        const long long f0 = (long long)f * frame;
        const int count = (int)((long long)len - f0 < frame ? (long long)len - f0 : frame);
        const float* x = wav + row + f0;
        const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
        float acc = 0.f;
        for (int q = lane * 4; q < count; q += 256) {
            float v0, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            if (aligned && q + 3 < count) {
                const float4 v = *reinterpret_cast<const float4*>(x + q);
                v0 = v.x; v1 = v.y; v2 = v.z; v3 = v.w;
            } else {
                v0 = x[q];
                if (q + 1 < count) v1 = x[q + 1];
                if (q + 2 < count) v2 = x[q + 2];
                if (q + 3 < count) v3 = x[q + 3];
            }
            acc += v0 * v0; acc += v1 * v1; acc += v2 * v2; acc += v3 * v3;
        }
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == 0 && acc >= thr2 * (float)count) {
            atomicMin(&s_first, f);
            atomicMax(&s_last, f);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int begin = 0, end = 0;
        if (s_last >= 0) {
            const long long lo = (long long)s_first * frame - keep, hi = ((long long)s_last + 1) * frame + keep;
            begin = (int)(lo < 0 ? 0 : lo);
            end = (int)(hi > len ? len : hi);
        }
        edges[2 * b] = begin;
        edges[2 * b + 1] = end;
    }
}

struct JoinTable {
    int begin[JOIN_ROWS], count[JOIN_ROWS], offset[JOIN_ROWS];
};

// the weight of sample i of a span of `count` samples under a fade of n <= count / 2 samples: (2 i + 1) / (2 n) over the first n, its
// mirror image over the last n - ONE correctly rounded fp32 division of two integers that fp32 holds exactly - and 1 in between
__device__ __forceinline__ float join_sample(const float* __restrict__ src, int i, int count, int n) {
    const float x = src[i];
    const int k = i < n ? i : (i >= count - n ? count - 1 - i : -1);
    if (k < 0) return x;
    return x * ((float)(2 * k + 1) / (float)(2 * n));
}

// out[offset[b] + i] = wav[b, begin[b] + i] w_b(i) for i < count[b]; every other sample of out is +0.0 (the pauses).  A thread writes
// the 4 consecutive samples 4 t .. 4 t + 3 with one 16-byte store (out is 16-byte aligned; the tail of out with scalar stores).  The
// spans are ascending and disjoint, so a sample belongs to at most one row: no atomics, every sample of out is written exactly once.
__global__ __launch_bounds__(JOIN_THREADS) void wav_join_kernel(const float* __restrict__ wav, int stride, JoinTable tab, int B, int fade,
                                                                 int total, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long j0 = ((long long)blockIdx.x * JOIN_THREADS + threadIdx.x) * 4;
    if (j0 >= total) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
        const int off = tab.offset[b], count = tab.count[b];
        if ((long long)off + count <= j0 || off >= j0 + 4) continue;
        const float* src = wav + (size_t)b * stride + tab.begin[b];
        const int n = fade < count / 2 ? fade : count / 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long i = j0 + e - off;
            if (i >= 0 && i < count) v[e] = join_sample(src, (int)i, count, n);
        }
    }
    if (j0 + 3 < total) {
        *reinterpret_cast<float4*>(out + j0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; j0 + e < total; ++e) out[j0 + e] = v[e];
    }
}

}  // namespace

// wav [B, stride] device, lens_host [B] in 0 .. stride, edges [B, 2] device int (begin, end) in samples; a row with no loud frame: (0, 0)
void Model::wav_edges(const float* wav, const int* lens_host, int B, int stride, int frame, float threshold, int keep, int* edges,
                      hipStream_t s) {
    DTTS_REQUIRE(wav && lens_host && edges, "wav_edges: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 1, "wav_edges: B, stride");
    DTTS_REQUIRE(frame >= 1 && keep >= 0, "wav_edges: frame >= 1, keep >= 0");
    DTTS_REQUIRE(std::isfinite(threshold) && threshold >= 0.f && std::isfinite(threshold * threshold * (float)frame),
                 "wav_edges: threshold has to be finite and >= 0");
    for (int b = 0; b < B; ++b) DTTS_REQUIRE(lens_host[b] >= 0 && lens_host[b] <= stride, "wav_edges: lens[b] in 0 .. stride");
    for (int b0 = 0; b0 < B; b0 += JOIN_ROWS) {       // the lengths travel as a kernel argument, 16 rows a launch: no upload, no table
        const int nb = B - b0 < JOIN_ROWS ? B - b0 : JOIN_ROWS;
        EdgeLens lens = {};
        for (int b = 0; b < nb; ++b) lens.len[b] = lens_host[b0 + b];
        hipLaunchKernelGGL(wav_edges_kernel, dim3(nb), dim3(EDGE_THREADS), 0, s, wav + (size_t)b0 * stride, lens, stride, frame,
                           threshold * threshold, keep, edges + 2 * b0);
        DTTS_CHECK_HIP(hipGetLastError());
    }
}

// wav [B, stride] device, begins / counts / offsets HOST [B], out [total] device (not aliasing wav); every sample of out is written
void Model::wav_join(const float* wav, int B, int stride, const int* begins, const int* counts, const int* offsets, long long total,
                     int fade, float* out, hipStream_t s) {
    DTTS_REQUIRE(wav && begins && counts && offsets, "wav_join: null argument");
    DTTS_REQUIRE(B >= 1 && B <= JOIN_ROWS, "wav_join: B in 1 .. 16");
    DTTS_REQUIRE(stride >= 1 && fade >= 0 && fade <= (1 << 23), "wav_join: stride >= 1, fade in 0 .. 2**23 (2 n exact in fp32)");
    DTTS_REQUIRE(total >= 0 && total < (1ll << 31), "wav_join: total in 0 .. 2**31 - 1");
    JoinTable tab = {};
    long long at = 0;
    for (int b = 0; b < B; ++b) {
        DTTS_REQUIRE(begins[b] >= 0 && counts[b] >= 0 && (long long)begins[b] + counts[b] <= stride,
                     "wav_join: begins[b] + counts[b] <= stride");
        DTTS_REQUIRE(offsets[b] >= at, "wav_join: the spans [offsets[b], offsets[b] + counts[b]) have to be ascending and disjoint");
        at = (long long)offsets[b] + counts[b];
        tab.begin[b] = begins[b]; tab.count[b] = counts[b]; tab.offset[b] = offsets[b];
    }
    DTTS_REQUIRE(at <= total, "wav_join: the last span ends beyond total");
    if (total == 0) return;
    DTTS_REQUIRE(out, "wav_join: out");
    const long long quads = (total + 3) / 4;
    hipLaunchKernelGGL(wav_join_kernel, dim3((unsigned)((quads + JOIN_THREADS - 1) / JOIN_THREADS)), dim3(JOIN_THREADS), 0, s, wav, stride,
                       tab, B, fade, (int)total, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
