// Speaking-rate control in stage B: the frame -> code map of every row, and the code embedding's affine read through it.
//
// The reference expands the code embedding [B,768,n] to ANY frame count T with F.interpolate(size=T, mode='nearest')
// (vqvae/diff_model.py:252); do_spectrogram_diffusion fixes T = 4 n, where the map is t / 4 (ops.hip affine_apply_kernel, up = 4:
// that launch stays the default path).  Here a row b has n_b codes and T_b frames, and a map m_b[0 .. T_b) into [0, n_b):
//   frame_map_uniform_kernel     F.interpolate's own rule (below)
//   frame_map_durations_kernel   repeat_interleave(arange(n_b), durations_b): code j owns durations_b[j] consecutive frames
//   affine_gather_kernel         y[b][c][t] = a_bc x[b][c][m_b[t]] + d_bc, the expression of affine_apply_kernel with m_b[t] for t / up
// Plain fp32 / int32; no atomics; every result is independent of the launch geometry (the scan is over integers).
#include "ops.h"
#include "model.h"

namespace dtts {

constexpr int FM_THREADS = 256;

// torch's nearest rule (ATen UpSample.h, nearest_neighbor_compute_source_index with compute_scales_value = in / out):
//     scale = float(n) / float(T);   m[t] = min((int)floorf(float(t) * scale), n - 1)
// in FLOAT32 with the division and the product each rounded ONCE.  It is not floor(t n / T): the two differ, e.g. at (n, T, t) =
// (14, 92, 46), (26, 44, 22), (12, 148, 37) - t n / T is an integer there and the rounded scale falls just below it - and a
// reciprocal-multiply (t n (1 / T)) differs again, e.g. at (6, 148).  A frame on the wrong code is a wrong column of the embedding,
// so the rule is reproduced to the bit: a correctly rounded divide, a separately rounded product, no contraction, no fast divide,
// no reciprocal.  At T = 4 n the scale is exactly 0.25 and the rule is t / 4.
__device__ __forceinline__ int nearest_source_index(int t, int n, int T) {
#pragma clang fp contract(off)
    const float scale = __fdiv_rn((float)n, (float)T);
    const int m = (int)floorf(__fmul_rn((float)t, scale));
    return m < n - 1 ? m : n - 1;
}

// grid (cdiv(Tmax, FM_THREADS), B): map[b][t] for t < frames[b], -1 beyond
__global__ __launch_bounds__(FM_THREADS) void frame_map_uniform_kernel(const int* __restrict__ lens_n, const int* __restrict__ frames,
                                                                       int Tmax, int* __restrict__ map) {
    const int b = blockIdx.y;
    const int n = lens_n[b], T = frames[b];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < Tmax; t += gridDim.x * blockDim.x)
        map[(long long)b * Tmax + t] = t < T ? nearest_source_index(t, n, T) : -1;
}

// grid (B), one workgroup per row.  The row's durations are scanned chunk by chunk (FM_THREADS codes at a time, an inclusive
// Hillis-Steele scan in LDS, the running total carried in a register every thread holds); after a chunk's scan its codes own the
// frames [carry, carry + chunk total), and every such frame finds its code by an upper-bound search in the chunk's prefix sums - a
// code of duration 0 owns no frame and is never found.  Writes are coalesced along t.  Frames at and beyond the row's total: -1.
__global__ __launch_bounds__(FM_THREADS) void frame_map_durations_kernel(const int* __restrict__ lens_n, const int* __restrict__ durations,
                                                                         int nmax, int Tmax, int* __restrict__ map) {
    __shared__ int incl[FM_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = lens_n[b];
    const int* d = durations + (long long)b * nmax;
    int* row = map + (long long)b * Tmax;
    int carry = 0;                                            // frames owned by the codes in front of this chunk
    for (int c0 = 0; c0 < n; c0 += FM_THREADS) {
        const int j = c0 + tid;
        incl[tid] = j < n ? d[j] : 0;
        __syncthreads();
        for (int o = 1; o < FM_THREADS; o <<= 1) {
            const int add = tid >= o ? incl[tid - o] : 0;
            __syncthreads();
            incl[tid] += add;
            __syncthreads();
        }
        const int total = incl[FM_THREADS - 1];
        for (int f = tid; f < total && carry + f < Tmax; f += FM_THREADS) {
            int lo = 0, hi = FM_THREADS - 1;                  // the first k with incl[k] > f (it exists: f < total)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (incl[mid] > f) hi = mid; else lo = mid + 1;
            }
            row[carry + f] = c0 + lo;
        }
        carry += total;
        __syncthreads();                                      // the next chunk overwrites incl
    }
    for (int t = carry + tid; t < Tmax; t += FM_THREADS) row[t] = -1;
}

// grid (<= 8, C, B) as affine_apply_kernel: y[b][c][t] = a x[b][c][map[b][t]] + d for t < frames[b]; columns beyond stay the caller's
__global__ __launch_bounds__(FM_THREADS) void affine_gather_kernel(const float* __restrict__ x, long long x_bs, int x_cs,
                                                                   const float* __restrict__ ab, const int* __restrict__ frames,
                                                                   const int* __restrict__ map, int Tmax, int C, float* __restrict__ y,
                                                                   long long y_bs, int y_cs) {
    const int c = blockIdx.y, b = blockIdx.z;
    const int len = frames[b];
    const float a = ab[((long long)b * C + c) * 2], d = ab[((long long)b * C + c) * 2 + 1];
    const float* xr = x + (long long)b * x_bs + (long long)c * x_cs;
    const int* mr = map + (long long)b * Tmax;
    float* yr = y + (long long)b * y_bs + (long long)c * y_cs;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < len; t += gridDim.x * blockDim.x)
        yr[t] = act_apply(a * xr[mr[t]] + d, ACT_NONE, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the arguments every entry shares, checked before any launch: lens_n[b] in 1 .. nmax, frames[b] in 1 .. Tmax, Tmax a multiple of
// 4 (the vocoder's x4 stages and infer_flowvae's assert, vqvae/model_24k.py), durations >= 0 with the row's sum == frames[b]
void Model::check_frames(const int* lens_n, const int* frames, const int* durations, int B, int nmax, int Tmax) {
    DTTS_REQUIRE(frames, "frame map: frames");
    DTTS_REQUIRE(B >= 1 && B <= 65535 && nmax >= 1, "frame map: B in 1 .. 65535, nmax >= 1");
    DTTS_REQUIRE(Tmax >= 4 && Tmax % 4 == 0, "frame map: Tmax has to be a positive multiple of 4");
    for (int b = 0; b < B; ++b) {
        const int n = lens_n ? lens_n[b] : nmax;
        DTTS_REQUIRE(n >= 1 && n <= nmax, "frame map: lens_n[b] in 1 .. nmax");
        DTTS_REQUIRE(frames[b] >= 1 && frames[b] <= Tmax, "frame map: frames[b] in 1 .. Tmax");
        if (!durations) continue;
        long long sum = 0;
        for (int j = 0; j < n; ++j) {
            DTTS_REQUIRE(durations[(size_t)b * nmax + j] >= 0, "frame map: durations >= 0");
            sum += durations[(size_t)b * nmax + j];
        }
        DTTS_REQUIRE(sum == frames[b], "frame map: a row's durations have to sum to frames[b]");
    }
}

// the row maps [B, Tmax] from lens_n / frames already on the device (durations are uploaded here, as lengths are)
void Model::frame_map_device(const int* d_lens_n, const int* d_frames, const int* durations_host, int B, int nmax, int Tmax, int* map,
                             hipStream_t s) {
    if (durations_host) {
        const int* dd = upload_ints(durations_host, B * nmax, s);
        hipLaunchKernelGGL(frame_map_durations_kernel, dim3(B), dim3(FM_THREADS), 0, s, d_lens_n, dd, nmax, Tmax, map);
    } else {
        hipLaunchKernelGGL(frame_map_uniform_kernel, dim3(cdiv(Tmax, FM_THREADS), B), dim3(FM_THREADS), 0, s, d_lens_n, d_frames, Tmax, map);
    }
    DTTS_CHECK_HIP(hipGetLastError());
}

void Model::op_frame_map(const int* lens_n_host, const int* frames_host, const int* durations_host, int B, int nmax, int Tmax, int* map_out,
                         hipStream_t s) {
    DTTS_REQUIRE(map_out, "op_frame_map: map_out");
    check_frames(lens_n_host, frames_host, durations_host, B, nmax, Tmax);
    std::vector<int> ln(B);
    for (int b = 0; b < B; ++b) ln[b] = lens_n_host ? lens_n_host[b] : nmax;
    const int* dl = upload_ints(ln.data(), B, s);
    const int* df = upload_ints(frames_host, B, s);
    frame_map_device(dl, df, durations_host, B, nmax, Tmax, map_out, s);
}

void Model::affine_gather(const float* x, long long x_bs, int x_cs, const float* ab, const int* d_frames, const int* map, int Tmax, int B,
                          int C, float* y, hipStream_t s) {
    dim3 grid(cdiv(Tmax, FM_THREADS) > 8 ? 8 : cdiv(Tmax, FM_THREADS), C, B);
    hipLaunchKernelGGL(affine_gather_kernel, grid, dim3(FM_THREADS), 0, s, x, x_bs, x_cs, ab, d_frames, map, Tmax, C, y,
                       (long long)C * Tmax, Tmax);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
