// Voices: the prompt's latents as values of their own (detail_tts_amd/voice.py).  The encoders that make them are the ones every request
// ran so far (mel_style, diff_conditioning); what is new is the pool over the n clips of a speaker - UnifiedVoice.get_conditioning's
// conds.mean(dim=1) (gpt/model.py:419-427), DiffusionTts.get_conditioning's mean over the concatenated embedder outputs
// (vqvae/diff_model.py:221-229) - and the convex blend of two voices, which is the same sum.
#include <cmath>

#include "model.h"

namespace dtts {

// out[s, d] = sum_j w[s, j] v[s, j, d] / sum_j w[s, j], fp32, j ascending, every product, sum and the quotient rounded on its own
// (nothing contracted to an fma).  One thread per (s, d), no atomics: two calls give the same bits.  w == nullptr: every weight 1.
// Clips of weight 0 are skipped (they contribute nothing, whatever they hold), and a speaker with ONE live clip - n = 1 above all - is
// not pooled: its bits are copied, so a voice made of one clip is the encoder's output bit for bit (w v / w would not be).
// Plain * and + under `fp contract(off)`: HIP's __fmul_rn / __fadd_rn are inline functions compiled under the default contraction
// mode, and behind them the compiler still emitted v_fmac_f32 for acc + w x here.
__global__ void voice_pool_kernel(const float* __restrict__ v, const float* __restrict__ w, int n, int D, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int s = blockIdx.y, d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const float* vs = v + (size_t)s * n * D + d;
    const float* wr = w ? w + (size_t)s * n : nullptr;
    float acc = 0.f, wsum = 0.f, one = 0.f;
    int live = 0;
    for (int j = 0; j < n; ++j) {
        const float wj = wr ? wr[j] : 1.f;
        if (wj == 0.f) continue;
        const float x = vs[(size_t)j * D];
        const float t = wj * x;
        acc = live ? acc + t : t;
        wsum = live ? wsum + wj : wj;
        one = x;
        ++live;
    }
    out[(size_t)s * D + d] = live == 1 ? one : acc / wsum;
}

// v [S, n, D] device, w_host [S][n] or nullptr (all 1), out [S, D] device (not aliasing v).  Weights are checked here, on the host
// where they live, before the launch: finite, >= 0, every speaker's sum > 0.
void Model::voice_pool(const float* v, const float* w_host, int S, int n, int D, float* out, hipStream_t s) {
    DTTS_REQUIRE(v && out, "voice_pool: null argument");
    DTTS_REQUIRE(S >= 1 && n >= 1 && D >= 1 && S <= 65535 && (long long)S * n <= (1 << 16), "voice_pool: S, n, D");
    const float* dw = nullptr;
    if (w_host) {
        for (int i = 0; i < S; ++i) {
            double sum = 0.0;
            for (int j = 0; j < n; ++j) {
                const float x = w_host[(size_t)i * n + j];
                DTTS_REQUIRE(std::isfinite(x) && x >= 0.f, "voice_pool: weights have to be finite and >= 0");
                sum += x;
            }
            DTTS_REQUIRE(sum > 0.0, "voice_pool: a speaker's weights sum to 0");
        }
        static_assert(sizeof(float) == sizeof(int), "weights travel through the int upload ring");
        dw = reinterpret_cast<const float*>(upload_ints(reinterpret_cast<const int*>(w_host), S * n, s));
    }
    hipLaunchKernelGGL(voice_pool_kernel, dim3(cdiv(D, 256), S), dim3(256), 0, s, v, dw, n, D, out);
    DTTS_CHECK_HIP(hipGetLastError());
}

}  // namespace dtts
