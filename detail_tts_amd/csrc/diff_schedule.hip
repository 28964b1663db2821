// Diffusion schedule arithmetic (diff_schedule.h): pure host code, no HIP call.
#include "diff_schedule.h"

#include <cmath>

namespace dtts {

// ---- diffusion schedule (float64 on the host, cast to fp32 on use: vqvae/utils/diffusion.py:179-228, 1181-1195, 1315)
// space_timesteps(trained, [steps])  (vqvae/utils/diffusion.py:1223-1272)
std::vector<int> space_steps(int trained, int steps) {
    std::vector<char> use(trained, 0);
    const double frac = steps <= 1 ? 1.0 : (double)(trained - 1) / (double)(steps - 1);
    double cur = 0.0;
    for (int i = 0; i < steps; ++i) {
        use[(int)std::nearbyint(cur)] = 1;   // Python round(): half to even == nearbyint in the default mode
        cur += frac;
    }
    std::vector<int> tmap;
    for (int i = 0; i < trained; ++i)
        if (use[i]) tmap.push_back(i);
    return tmap;
}

// the spaced schedule of the model timesteps `tmap` (ascending, distinct, in [0, trained))
void make_schedule(int trained, const std::vector<int>& tmap, float cfk_k, ScheduleTables& sc) {
    std::vector<double> betas(trained), ac(trained);
    const double scale = 1000.0 / trained, b0 = scale * 0.0001, b1 = scale * 0.02;
    double prod = 1.0;
    for (int i = 0; i < trained; ++i) {
        betas[i] = trained > 1 ? b0 + (b1 - b0) * (double)i / (double)(trained - 1) : b0;
        prod *= (1.0 - betas[i]);
        ac[i] = prod;
    }
    std::vector<double> nb;
    double last = 1.0;
    for (int t : tmap) {
        nb.push_back(1.0 - ac[t] / last);
        last = ac[t];
    }
    const int n = (int)nb.size();
    std::vector<double> acp(n), acp_prev(n), post_var(n);
    prod = 1.0;
    for (int i = 0; i < n; ++i) {
        acp_prev[i] = prod;
        prod *= (1.0 - nb[i]);
        acp[i] = prod;
    }
    for (int i = 0; i < n; ++i) post_var[i] = nb[i] * (1.0 - acp_prev[i]) / (1.0 - acp[i]);
    sc.tmap = tmap;
    sc.n = n;
    sc.cfk_k = cfk_k;
    sc.p.resize(n);
    sc.ac.resize(n);
    sc.ac_prev.resize(n);
    sc.ac_next.resize(n);
    sc.sqrt_ac.resize(n);
    sc.sqrt_1m_ac.resize(n);
    sc.log_1m_ac.resize(n);
    sc.ac64 = acp;
    for (int i = 0; i < n; ++i) {
        DiffStepCoefs k;
        k.sqrt_recip_ac = (float)std::sqrt(1.0 / acp[i]);
        k.sqrt_recipm1_ac = (float)std::sqrt(1.0 / acp[i] - 1.0);
        k.coef1 = (float)(nb[i] * std::sqrt(acp_prev[i]) / (1.0 - acp[i]));
        k.coef2 = (float)((1.0 - acp_prev[i]) * std::sqrt(1.0 - nb[i]) / (1.0 - acp[i]));
        // posterior_log_variance_clipped; a 1-step schedule has no post_var[1] (the reference cannot build one) and never uses it
        k.min_log = (float)std::log(i == 0 ? post_var[n > 1 ? 1 : 0] : post_var[i]);
        k.max_log = (float)std::log(nb[i]);
        k.cfk = (float)(cfk_k * (1.0 - (double)i / (double)n));
        k.nonzero = i != 0;
        sc.p[i] = k;
        sc.ac[i] = (float)acp[i];
        sc.ac_prev[i] = (float)acp_prev[i];
        sc.ac_next[i] = i + 1 < n ? (float)acp[i + 1] : 0.f;              // np.append(alphas_cumprod[1:], 0.0)
        sc.sqrt_ac[i] = (float)std::sqrt(acp[i]);
        sc.sqrt_1m_ac[i] = (float)std::sqrt(1.0 - acp[i]);
        sc.log_1m_ac[i] = (float)std::log(1.0 - acp[i]);
    }
}

// ddim_sample's scalars (vqvae/utils/diffusion.py:773-777) in fp32, as the reference evaluates them on fp32 tensors
DdimStepCoefs ScheduleTables::ddim(int i, float eta) const {
    DdimStepCoefs k;
    k.sqrt_recip_ac = p[i].sqrt_recip_ac;
    k.sqrt_recipm1_ac = p[i].sqrt_recipm1_ac;
    k.cfk = p[i].cfk;
    const float a = ac[i], ap = ac_prev[i];
    k.sigma = eta * std::sqrt((1.f - ap) / (1.f - a)) * std::sqrt(1.f - a / ap);
    k.sqrt_ac_prev = std::sqrt(ap);
    k.dir = std::sqrt(1.f - ap - k.sigma * k.sigma);
    k.nonzero = i != 0;
    return k;
}

// ddim_reverse_sample's scalars (vqvae/utils/diffusion.py:809-815): alphas_cumprod_next is cast to fp32 by _extract_into_tensor, then
// th.sqrt and 1 - . run on the fp32 tensor
DdimReverseCoefs ScheduleTables::ddim_reverse(int i) const {
    DdimReverseCoefs k;
    k.sqrt_recip_ac = p[i].sqrt_recip_ac;
    k.sqrt_recipm1_ac = p[i].sqrt_recipm1_ac;
    k.cfk = p[i].cfk;
    const float an = ac_next[i];
    k.sqrt_ac_next = std::sqrt(an);
    k.sqrt_1m_ac_next = std::sqrt(1.f - an);
    return k;
}

// The inpainting step's scalars (diff_inpaint.h): the known frames at level i - 1 are q_sample at alphas_cumprod_prev[i], and a repeat
// goes back up by one forward step of beta_i = 1 - ac[i] / acp[i].  Double throughout, one rounding to fp32 each.
InpaintCoefs ScheduleTables::inpaint(int i) const {
    const double a = ac64[i], ap = i > 0 ? ac64[i - 1] : 1.0;
    InpaintCoefs k;
    k.known_a = (float)std::sqrt(ap);
    k.known_b = (float)std::sqrt(1.0 - ap);
    k.renoise_a = (float)std::sqrt(a / ap);
    k.renoise_b = (float)std::sqrt(1.0 - a / ap);
    return k;
}

// ---- DPM-Solver++(2M) (vqvae/utils/diffusion.py:487-581 -> vqvae/utils/dpm_solver.py), fp32 scalars in the reference's order
// NoiseScheduleVP("linear", continuous_beta_0 = 0.1 / 4, continuous_beta_1 = 20 / 4) (:108-154): the Python float constants meet fp32
// 0-d tensors, so each is rounded to fp32 and every operation is rounded on its own
static float dpm_log_alpha(float t) {               // marginal_log_mean_coeff: -0.25 t^2 (b1 - b0) - 0.5 t b0
#pragma clang fp contract(off)
    const float a = (-0.25f * (t * t)) * (float)(20.0 / 4 - 0.1 / 4);
    const float b = (0.5f * t) * (float)(0.1 / 4);
    return a - b;
}
static float dpm_sigma(float t) { return std::sqrt(1.f - std::exp(2.f * dpm_log_alpha(t))); }       // marginal_std
static float dpm_lambda(float t) {                                                                 // marginal_lambda
#pragma clang fp contract(off)
    const float la = dpm_log_alpha(t);
    return la - 0.5f * std::log(1.f - std::exp(2.f * la));
}

void dpm_schedule_table(int n, float cfk, std::vector<float>& times, std::vector<float>& model_times, std::vector<DpmStepCoefs>& steps,
                        std::vector<float>* lambda_s) {
#pragma clang fp contract(off)
    DTTS_REQUIRE(n >= 2, "DPM-Solver++(2M) needs at least 2 steps (the reference asserts steps >= order)");
    // torch.linspace(t_T = 1, t_0 = 1 / total_N, n + 1) in fp32 (:474, 1159-1173) as torch's CPU kernel fills it: the first half
    // start + step * i, the second half end - step * (n - i), each a fused multiply-add
    const float start = 1.f, end = (float)(1.0 / 1000), step = (end - start) / (float)n;
    const int cnt = n + 1, half = cnt / 2;
    times.resize(cnt);
    for (int i = 0; i < cnt; ++i)
        times[i] = i < half ? std::fma(step, (float)i, start) : std::fma(-step, (float)(cnt - 1 - i), end);
    model_times.resize(n);
    steps.resize(n);
    if (lambda_s) lambda_s->resize(n);
    for (int k = 0; k < n; ++k) {
        const float s = times[k], t = times[k + 1];
        model_times[k] = s * 1000.f;                                    // t_continuous * 1000 (vqvae/utils/diffusion.py:534)
        DpmStepCoefs c;
        c.cfk = cfk;
        c.alpha_s = std::exp(dpm_log_alpha(s));
        c.sigma_s = dpm_sigma(s);
        const float lam_s = dpm_lambda(s), lam_t = dpm_lambda(t);
        const float h = lam_t - lam_s;
        c.ratio = dpm_sigma(t) / c.sigma_s;
        c.c1 = std::exp(dpm_log_alpha(t)) * std::expm1(-h);
        c.c2 = 0.5f * c.c1;
        // the first step is first order; so is the last one below 10 steps (lower_order_final, :1195-1201)
        c.order = (k == 0 || (n < 10 && k == n - 1)) ? 1 : 2;
        c.inv_r0 = 0.f;
        if (c.order == 2) {
            const float h_0 = lam_s - dpm_lambda(times[k - 1]);
            c.inv_r0 = 1.f / (h_0 / h);
        }
        steps[k] = c;
        if (lambda_s) (*lambda_s)[k] = lam_s;
    }
}

}  // namespace dtts
