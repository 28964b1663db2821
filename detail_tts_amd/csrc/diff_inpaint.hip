// Mel inpainting in the diffusion decoder: the blend kernel of Model::diff_inpaint (diff_inpaint.h).
#include "diff_inpaint.h"
#include "philox.h"

namespace dtts {

// Steps 2 - 4 of an inpainting step in one pass (see diff_inpaint.h).  Same element walk and ragged lens as diff_update_kernel, so a
// row's noise never depends on the batch's padding.  No contraction: the NumPy fp32 restatement (tests/inpaint_ref.py) rounds every
// product and the sum on their own, and the test compares bit for bit.
__global__ void inpaint_blend_kernel(float* x, const float* known, const unsigned char* keep, const int* lens, int T, int B, int C,
                                     InpaintCoefs k, int step0, int renoise, unsigned long long seed, const int* sample_ids, int pstep,
                                     const float* known_noise, const float* renoise_noise) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int len = lens ? lens[b] : T;
    const long long base = (long long)b * C * T;
    const unsigned char* kb = keep + (long long)b * T;
    const bool draw_known = !step0 && !known_noise, draw_renoise = renoise && !renoise_noise;
    const unsigned sample = (draw_known || draw_renoise) ? (unsigned)sample_ids[b] : 0u;
    const int n = C * len;
    const int nblk = (n + 3) / 4;
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nblk; blk += gridDim.x * blockDim.x) {
        float zk[4] = {0.f, 0.f, 0.f, 0.f}, zr[4] = {0.f, 0.f, 0.f, 0.f};
        if (draw_known) philox_normal4(seed, sample, STAGE_DIFF_KNOWN, pstep, (unsigned)blk, zk);
        if (draw_renoise) philox_normal4(seed, sample, STAGE_DIFF_RENOISE, pstep, (unsigned)blk, zr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = blk * 4 + i;
            if (e >= n) break;
            const int c = e / len, t = e - c * len;
            const long long o = base + (long long)c * T + t;
            const bool kept = kb[t] != 0;
            if (!kept && !renoise) continue;                           // the sampler's update stands
            float v;
            if (kept) {
                const float kv = known[o];
                v = step0 ? kv : k.known_a * kv + k.known_b * (known_noise ? known_noise[o] : zk[i]);
            } else {
                v = x[o];
            }
            if (renoise) v = k.renoise_a * v + k.renoise_b * (renoise_noise ? renoise_noise[o] : zr[i]);
            x[o] = v;
        }
    }
}

void launch_inpaint_blend(float* x, const float* known, const unsigned char* keep, const int* lens, int T, int B, int C, InpaintCoefs k,
                          int step0, int renoise, unsigned long long seed, const int* sample_ids, int pstep, const float* known_noise,
                          const float* renoise_noise, hipStream_t s) {
    DTTS_REQUIRE(x && known && keep && B >= 1 && B <= 65535 && C >= 1 && T >= 1 && (long long)C * T < (1ll << 31) - 4,
                 "inpaint blend: x, known, keep; 1 <= B <= 65535; C * T below 2^31");
    DTTS_REQUIRE(!(step0 && renoise), "inpaint blend: step 0 is never repeated");
    DTTS_REQUIRE(sample_ids || ((step0 || known_noise) && (!renoise || renoise_noise)), "inpaint blend: sample_ids or the noise arrays");
    const int nblk = (C * T + 3) / 4;
    hipLaunchKernelGGL(inpaint_blend_kernel, dim3(cdiv(nblk, 256) > 64 ? 64 : cdiv(nblk, 256), B), dim3(256), 0, s, x, known, keep, lens, T,
                       B, C, k, step0, renoise, seed, sample_ids, pstep, known_noise, renoise_noise);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
