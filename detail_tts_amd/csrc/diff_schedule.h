// Sampling schedules of the diffusion stage: the host arithmetic (diff_schedule.hip, no HIP call) and the Schedule the runtime caches.
#pragma once
#include <vector>

#include "diff_inpaint.h"
#include "ops.h"

namespace dtts {

// The host tables of a sampling schedule: SpacedDiffusion(use_timesteps = tmap, linear betas over cfg.diff_trained_steps)
// (vqvae/utils/diffusion.py:1172-1220), computed in float64 and cast to fp32.
// Float-time schedules (kind != 0) carry fp32 model times instead of tmap: DPM-Solver++(2M) of n steps (kind 1: k_diffusion_sample_loop,
// vqvae/utils/diffusion.py:487-581), or fractional forward times alone (kind 2: diff_forward_tf).  Column i of every table is step
// n - 1 - i of the loop (n - 1 = first), as for the integer schedules, so the samplers' loop and the trunk read them the same way.
struct ScheduleTables {
    int kind = 0;                         // 0: integer timesteps (tmap); 1: DPM-Solver++(2M); 2: fractional model times (forward only)
    std::vector<int> tmap;                // kind 0: model timesteps of the spaced steps, ascending (timestep_map)
    std::vector<float> ftimes;            // kinds 1, 2: fp32 model time of column i, ascending (kind 1: t_{n-1-i} * 1000)
    std::vector<DiffStepCoefs> p;         // ancestral sampler (p_sample)
    std::vector<float> ac, ac_prev;       // fp32 alphas_cumprod / alphas_cumprod_prev (DDIM: the eta-dependent terms are per call)
    std::vector<float> ac_next;           // kind 0: fp32 alphas_cumprod_next (ddim_reverse_sample, :812); 0 at the last step
    std::vector<float> sqrt_ac, sqrt_1m_ac;   // kind 0: fp32 sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod (q_sample, :243-260)
    std::vector<float> log_1m_ac;         // kind 0: fp32 log_one_minus_alphas_cumprod (q_mean_variance, :230-241: _prior_bpd)
    std::vector<DpmStepCoefs> dpm;        // kind 1: the update of column i
    std::vector<double> ac64;             // kind 0: float64 alphas_cumprod (inpaint: every scalar is rounded once, from these)
    float cfk_k = 0.f;
    int n = 0;
    DdimStepCoefs ddim(int i, float eta) const;
    DdimReverseCoefs ddim_reverse(int i) const;
    InpaintCoefs inpaint(int i) const;
    bool same_key(const ScheduleTables& o) const { return kind == o.kind && tmap == o.tmap && ftimes == o.ftimes; }
};

// A schedule on a handle: the host tables and ss_table, every ResBlock's AdaGN scale / shift at every step of the schedule:
// emb_layers(time_embed(sinusoid(tmap[i]))) (vqvae/diff_model.py:294, 108).  (model_diffusion.hip)
struct Schedule : ScheduleTables {
    int id = 0;                           // 0: the default (cfg.diff_steps) schedule built at bind
    const float* ss_table = nullptr;      // [n_resblocks][2C][n]
    void* mem = nullptr;                  // owned device memory (cached schedules; the default one lives in the bind-time arena)
    hipEvent_t used = nullptr;            // recorded after every call that read ss_table: an eviction waits for it
    ~Schedule();
};

// space_timesteps(trained, [steps])  (vqvae/utils/diffusion.py:1223-1272)
std::vector<int> space_steps(int trained, int steps);
// the spaced schedule of the model timesteps `tmap` (ascending, distinct, in [0, trained)): kind 0 tables of sc
void make_schedule(int trained, const std::vector<int>& tmap, float cfk_k, ScheduleTables& sc);

// DPM-Solver++(2M) of n >= 2 steps as the reference's DPM_Solver.sample runs it (vqvae/utils/dpm_solver.py:1159-1201: time_uniform,
// multistep, order 2, lower_order_final) on NoiseScheduleVP("linear", 0.025, 5.0) (:108-154), in fp32 in the reference's order of
// operations.  times [n + 1]: torch.linspace(1, 1e-3, n + 1) in fp32; model_times [n]: t_k * 1000; steps [n]: the update t_k -> t_{k+1}
// in the solver's order (k = 0 first); lambda_s [n] (optional): lambda(t_k).
void dpm_schedule_table(int n, float cfk, std::vector<float>& times, std::vector<float>& model_times, std::vector<DpmStepCoefs>& steps,
                        std::vector<float>* lambda_s = nullptr);

}  // namespace dtts
