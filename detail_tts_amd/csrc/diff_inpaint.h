// Mel inpainting in the diffusion decoder (RePaint, Lugmayr et al. 2022): the per-step blend of known and generated frames.
#pragma once
#include "common.h"

namespace dtts {

// The four scalars of one inpainting step i of a spaced schedule, from its float64 alphas_cumprod (ac) and alphas_cumprod_prev (acp,
// acp[0] = 1): each evaluated in double and rounded once to fp32 (ScheduleTables::inpaint).
struct InpaintCoefs {
    float known_a, known_b;       // the known frames at level i - 1: sqrt(acp[i]), sqrt(1 - acp[i])      (1, 0 at i = 0)
    float renoise_a, renoise_b;   // one forward step from level i - 1 back to level i: sqrt(ac[i] / acp[i]), sqrt(1 - ac[i] / acp[i])
};

// x [B][C][T] holds the sampler's update u at level i - 1 on entry and is rewritten in place:
//   k = known_a * known + known_b * eps_known         (step0: k = known, a copy)
//   x = keep[b][t] ? k : u                            (a select; `known` is read only where keep is set)
//   renoise: x = renoise_a * x + renoise_b * eps_renoise
// keep [B][T] bytes, one per frame.  The element walk is diff_update_kernel's (ops.hip): four elements per Philox block, the element
// index over the row's own [C, lens[b]], frames at or beyond lens[b] never touched.  eps_known / eps_renoise: the Philox streams
// STAGE_DIFF_KNOWN / STAGE_DIFF_RENOISE at step field `pstep`, or the dense [B][C][T] arrays known_noise / renoise_noise in their
// place.  No contraction: every line is two products and one sum, each rounded on its own.
void launch_inpaint_blend(float* x, const float* known, const unsigned char* keep, const int* lens, int T, int B, int C, InpaintCoefs k,
                          int step0, int renoise, unsigned long long seed, const int* sample_ids, int pstep, const float* known_noise,
                          const float* renoise_noise, hipStream_t s);

}  // namespace dtts
