// Common definitions for libdetail_hip.so (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace dtts {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define DTTS_CHECK_HIP(expr)                                                                  \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            throw ::dtts::Error(-2, std::string(#expr) + " failed: " + hipGetErrorString(_e) + \
                                        " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
    } while (0)

#define DTTS_REQUIRE(cond, msg)                                                      \
    do {                                                                             \
        if (!(cond))                                                                 \
            throw ::dtts::Error(-1, std::string("invalid argument: ") + (msg) +      \
                                        " [" #cond "] at " + __FILE__ + ":" + std::to_string(__LINE__)); \
    } while (0)

// Opt-in LDS sizes (hipFuncSetAttribute(MaxDynamicSharedMemorySize)) are a per-DEVICE property of a kernel: applied once per
// (device, kernel), under a lock, so that handles on several GPUs of one process and the stage threads of infer_stream are all served
// (device.hip).  lds_optin throws on failure; device_fits reports whether the current device can hold `wgs` co-resident workgroups
// of `lds_bytes` each, one per CU (the persistent kernels' requirement).
void lds_optin(const void* kernel, int bytes);
bool device_fits(int wgs, int lds_bytes);

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return cdiv(a, b) * b; }

// Environment switches (DTTS_*, DESIGN.md par. 4.10), host only.  One parsing for all of them; a call site caches what it reads in a
// `static const` (or, where dtts_set_option can override it later, reads lazily inside its getter).
static inline const char* env_str(const char* name) { return getenv(name); }       // the raw text, for the few switches with a parsing of their own
static inline long long env_int(const char* name, long long dflt) {
    const char* v = env_str(name);
    return v ? atoll(v) : dflt;
}
static inline bool env_on(const char* name) {          // on unless the value starts with '0'
    const char* v = env_str(name);
    return !(v && v[0] == '0');
}
static inline int env_tri(const char* name) {          // -1 = not set (the caller's own rule decides), else env_on
    return env_str(name) ? (env_on(name) ? 1 : 0) : -1;
}

// noise streams of the Philox spec (oracle/philox.py)
enum NoiseStage : int { STAGE_GPT_SAMPLE = 1, STAGE_DIFF_INIT = 2, STAGE_DIFF_STEP = 3, STAGE_FLOW_PRIOR = 4,
                        STAGE_DIFF_QSAMPLE = 5,     // 5: the forward process' noise (q_sample of the evaluation loss, diff_loss.h), step 0
                        STAGE_POSTERIOR = 6,        // 6: enc_q's posterior sample (forward_flowvae, flowvae_fwd.h), step 0
                        STAGE_DIFF_BPD = 7,         // 7: the forward process' noise of calc_bpd_loop (diff_bpd.h), step = timestep t
                        STAGE_DIFF_KNOWN = 8,       // 8: inpainting, the noise of the known frames (diff_inpaint.h), step = i + r * N
                        STAGE_DIFF_RENOISE = 9 };   // 9: inpainting, the forward step of a repeat, step = i + r * N

// activation ids shared by prologues / epilogues
enum Act : int {
    ACT_NONE = 0,
    ACT_SILU = 1,
    ACT_LRELU = 2,     // slope given separately
    ACT_RELU = 3,
    ACT_GELU_NEW = 4,
    ACT_TANH = 5,
    ACT_MISH = 6,
    ACT_LOG_CLAMP = 7, // log(max(v, 1e-5))   (dynamic_range_compression_torch, vqvae/utils/data_utils.py:21-27)
};

// epilogue pairing modes: packed weight rows (2r, 2r+1) hold the two halves of a gated pair
enum Gate : int {
    GATE_NONE = 0,
    GATE_TANH_SIGMOID = 1,   // tanh(a_r) * sigmoid(b_r)            (WN, modules.py:15-22)
    GATE_GLU = 2,            // a_r * sigmoid(b_r)                   (Conv1dGLU, modules.py:517-523)
};

__device__ __forceinline__ float act_apply(float v, int act, float slope) {
    switch (act) {
        case ACT_SILU: return v / (1.f + __expf(-v));
        case ACT_LRELU: return v >= 0.f ? v : v * slope;
        case ACT_RELU: return fmaxf(v, 0.f);
        case ACT_GELU_NEW: {
            float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
            return 0.5f * v * (1.f + tanhf(u));
        }
        case ACT_TANH: return tanhf(v);
        case ACT_MISH: {
            float sp = v > 20.f ? v : log1pf(expf(v));
            return v * tanhf(sp);
        }
        case ACT_LOG_CLAMP: return logf(fmaxf(v, 1e-5f));
        default: return v;
    }
}

// XCD-aware block remap (block i runs on XCD i % 8 on MI355X; used for L2 locality only, never for correctness):
// returns a logical block id such that each XCD owns one contiguous range of logical ids.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int i, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = i & 7, j = i >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }

}  // namespace dtts
