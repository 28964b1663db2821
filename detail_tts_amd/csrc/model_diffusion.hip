// Diffusion stage (stage B) of the model runtime: weights, schedule cache, trunk building blocks, entry points (see model.h).
#include "model.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <optional>
#include "prof.h"

namespace dtts {

// a stream whose queue is confined to the first `cus` CUs of the 256 (the mask's bits interleave over the 8 XCDs)
static void make_masked_stream(hipStream_t* st, int cus) {
    uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < cus; ++b) mask[b >> 5] |= 1u << (b & 31);
    DTTS_CHECK_HIP(hipExtStreamCreateWithCUMask(st, 8, mask));
}

// Side streams of the diffusion trunk.  DTTS_B_CU_RESERVE = n (experiment): the stream's queue is masked off the last n CUs of the
// 256, which stay free for the decode chain of the next request.
static void make_side_stream(hipStream_t* st) {
    static const int reserve = env_int("DTTS_B_CU_RESERVE", 0);
    if (reserve > 0 && reserve < 256) make_masked_stream(st, 256 - reserve);
    else DTTS_CHECK_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
}

void Model::ensure_fork_events() {
    if (ev_fork_) return;
    DTTS_CHECK_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
    for (auto& e : ev_joinx_) DTTS_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

// AdaGN tables of the schedule: t_emb = time_embed(sinusoid(ts)) for every sampling step, then every ResBlock's
// emb_layers (SiLU -> Linear) -> ss_table[rb][2C][NS]   (vqvae/diff_model.py:294, 108).  scratch: 3 C NS floats; ts_dev: NS words
void Model::build_ss_table(const Schedule& sc, float* ss_table, float* scratch, void* ts_dev, hipStream_t s) {
    const int C = cfg.diff_channels, NS = sc.n;
    float* sinus = scratch;
    float* t1 = scratch + (size_t)C * NS;
    float* temb = scratch + (size_t)2 * C * NS;
    if (sc.kind == 0) {
        DTTS_CHECK_HIP(hipMemcpyAsync(ts_dev, sc.tmap.data(), sizeof(int) * NS, hipMemcpyHostToDevice, s));
        launch_timestep_sinusoid(static_cast<const int*>(ts_dev), NS, C, sinus, s);
    } else {                                                   // fractional model times (timestep_embedding, vqvae/diff_model.py:20-38)
        DTTS_CHECK_HIP(hipMemcpyAsync(ts_dev, sc.ftimes.data(), sizeof(float) * NS, hipMemcpyHostToDevice, s));
        launch_timestep_sinusoid(static_cast<const float*>(ts_dev), NS, C, sinus, s);
    }
    ConvParams p = cp(sinus, C, t1, C, 1, NS, NS, nullptr);
    p.epi_act = ACT_SILU;
    run_conv(te0_, p, s);
    run_conv(te2_, cp(t1, C, temb, C, 1, NS, NS, nullptr), s);
    auto emb_of = [&](const ResBlockW& rb) {
        ConvParams q = cp(temb, C, ss_table + (size_t)rb.index * 2 * C * NS, 2 * C, 1, NS, NS, nullptr);
        q.pro_act = ACT_SILU;
        run_conv(rb.emb, q, s);
    };
    for (auto& l : integ_) emb_of(l.rb);
    for (auto& l : layers_) emb_of(l.rb);
    for (auto& r : tail_) emb_of(r);
}

Schedule::~Schedule() {
    if (used) (void)hipEventSynchronize(used);
    if (mem) (void)hipFree(mem);
    if (used) (void)hipEventDestroy(used);
}

Schedule& Model::schedule(int id) {
    if (id == 0) return sched0_;
    std::lock_guard<std::mutex> lk(sched_mu_);
    for (auto& e : sched_cache_)
        if (e->id == id) return *e;
    throw Error(-1, "diffusion schedule " + std::to_string(id) + " is not cached (evicted or never built): call dtts_diff_schedule again");
}

int Model::cache_schedule(std::unique_ptr<Schedule> sc, hipStream_t s) {
    std::lock_guard<std::mutex> lk(sched_mu_);
    for (size_t k = 0; k < sched_cache_.size(); ++k)
        if (sched_cache_[k]->same_key(*sc)) {
            std::rotate(sched_cache_.begin(), sched_cache_.begin() + k, sched_cache_.begin() + k + 1);   // most recently used first
            return sched_cache_[0]->id;
        }
    // evict the least recently used; its destructor waits for the last launch that read its table
    while (sched_cache_.size() >= MAX_SCHEDULES) sched_cache_.pop_back();
    const int C = cfg.diff_channels, NS = sc->n;
    const size_t fl = (size_t)n_resblocks_ * 2 * C * NS;
    DTTS_CHECK_HIP(hipMalloc(&sc->mem, sizeof(float) * (fl + 3 * (size_t)C * NS) + sizeof(int) * NS));
    float* base = static_cast<float*>(sc->mem);
    sc->ss_table = base;
    build_ss_table(*sc, base, base + fl, base + fl + 3 * (size_t)C * NS, s);
    DTTS_CHECK_HIP(hipEventCreateWithFlags(&sc->used, hipEventDisableTiming));
    DTTS_CHECK_HIP(hipEventRecord(sc->used, s));
    sc->id = sched_next_id_++;
    sched_cache_.insert(sched_cache_.begin(), std::move(sc));
    return sched_cache_[0]->id;
}

int Model::diff_schedule(const int* timesteps, int n, hipStream_t s) {
    DTTS_REQUIRE(bound_ && sched0_.n > 0, "diffusion weights not bound");
    DTTS_REQUIRE(timesteps && n >= 1, "diff_schedule: empty timestep list");
    const int trained = cfg.diff_trained_steps;
    std::vector<int> tmap(timesteps, timesteps + n);
    for (int t : tmap) DTTS_REQUIRE(t >= 0 && t < trained, "diff_schedule: timestep out of [0, diff_trained_steps)");
    std::sort(tmap.begin(), tmap.end());
    tmap.erase(std::unique(tmap.begin(), tmap.end()), tmap.end());
    if (tmap == sched0_.tmap) return 0;
    auto sc = std::make_unique<Schedule>();
    make_schedule(trained, tmap, cfg.cond_free_k, *sc);
    return cache_schedule(std::move(sc), s);
}

int Model::diff_schedule_dpm(int n, hipStream_t s) {
    DTTS_REQUIRE(bound_ && sched0_.n > 0, "diffusion weights not bound");
    DTTS_REQUIRE(n >= 2 && n <= cfg.diff_trained_steps, "diff_schedule_dpm: n out of [2, diff_trained_steps]");
    auto sc = std::make_unique<Schedule>();
    std::vector<float> times, mt;
    std::vector<DpmStepCoefs> steps;
    dpm_schedule_table(n, cfg.cond_free_k, times, mt, steps);
    sc->kind = 1;
    sc->n = n;
    sc->cfk_k = cfg.cond_free_k;
    sc->ftimes.resize(n);
    sc->dpm.resize(n);
    for (int i = 0; i < n; ++i) {                   // column i = solver step n - 1 - i
        sc->ftimes[i] = mt[n - 1 - i];
        sc->dpm[i] = steps[n - 1 - i];
    }
    return cache_schedule(std::move(sc), s);
}

int Model::diff_schedule_info(int sched_id, int* tmap, float* coefs, int cap) {
    const Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_schedule_coefs: not an integer-timestep schedule (DPM tables: dtts_dpm_schedule_table)");
    for (int i = 0; i < sc.n && i < cap; ++i) {
        if (tmap) tmap[i] = sc.tmap[i];
        if (coefs) {
            const DiffStepCoefs& k = sc.p[i];
            const float v[9] = {k.sqrt_recip_ac, k.sqrt_recipm1_ac, k.coef1, k.coef2, k.min_log, k.max_log, k.cfk, sc.ac[i], sc.ac_prev[i]};
            std::memcpy(coefs + (size_t)9 * i, v, sizeof(v));
        }
    }
    return sc.n;
}

// The x path of DiffusionTts.forward is two linear convs in a row (vqvae/diff_model.py:296-298: inp_block, k = 3, then the x columns of the
// 1 x 1 integrating_conv, no activation or norm between them), so they are ONE k = 3 conv whose weights depend on the checkpoint only:
//   W'[tap] = W1 . W_inp[tap],  b' = W1 . b_inp + b1        (packed layout [tap][ci][co]; W1 = integrating_conv.a)
// One thread per output element, the sum over the M middle channels in fp64, rounded once to fp32.  Row r < rows: weight row (tap, ci); row `rows`: the bias.
__global__ __launch_bounds__(256) void compose_xpath_kernel(const float* __restrict__ w_inp, const float* __restrict__ b_inp, int inp_ld,
                                                            const float* __restrict__ w1, const float* __restrict__ b1, int M, int CoutP,
                                                            int rows, float* __restrict__ w_out, float* __restrict__ b_out) {
    const int co = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (co >= CoutP) return;
    const float* a = r < rows ? w_inp + (size_t)r * inp_ld : b_inp;
    double acc = r < rows ? 0.0 : (double)b1[co];
    for (int m = 0; m < M; ++m) acc += (double)a[m] * (double)w1[(size_t)m * CoutP + co];
    (r < rows ? w_out + (size_t)r * CoutP : b_out)[co] = (float)acc;
}

void Model::build_diffusion(hipStream_t s) {
    const int C = cfg.diff_channels, H = cfg.diff_heads, NL = cfg.diff_layers;
    {
        std::lock_guard<std::mutex> lk(sched_mu_);
        sched_cache_.clear();                       // (re)bind: cached AdaGN tables were made of the previous weights
    }
    const std::string d = "diffusion.";
    integ_.clear();
    layers_.clear();
    tail_.clear();
    latcond_.clear();
    ctx_.clear();
    int rbi = 0;
    for (int i = 0; i < 3; ++i) {
        const std::string p = d + "conditioning_timestep_integrator." + std::to_string(i);
        integ_.push_back({res_block(p + ".resblk", C, rbi++), attn_block(p + ".attn", C, H)});
    }
    for (int i = 0; i < NL; ++i) {
        const std::string p = d + "layers." + std::to_string(i);
        layers_.push_back({res_block(p + ".resblk", C, rbi++), attn_block(p + ".attn", C, H)});
    }
    for (int i = NL; i < NL + 3; ++i) tail_.push_back(res_block(d + "layers." + std::to_string(i), C, rbi++));
    const PackedConv inp_block = conv(d + "inp_block", cfg.mel_channels, C, 3);
    const PackedConv integ1 = conv(d + "integrating_conv.a", C, C, 1);   // columns 0..C-1 of the 1x1 (x path) + bias: both only feed xpath_ below
    integ2_ = conv(d + "integrating_conv.b", C, C, 1, false);    // columns C..2C-1 (code path)
    out_gn_g_ = W(d + "out.0.weight", C);
    out_gn_b_ = W(d + "out.0.bias", C);
    out_conv_ = conv(d + "out.2", C, cfg.diff_out_channels, 3);
    code_gn_g_ = W(d + "code_norm.weight", C);
    code_gn_b_ = W(d + "code_norm.bias", C);
    uncond_ = W(d + "unconditioned_embedding", C);
    latcond0_ = conv(d + "latent_conditioner.0", C, C, 3);
    for (int i = 1; i < 5; ++i) latcond_.push_back(attn_block(d + "latent_conditioner." + std::to_string(i), C, H));
    ctx0_ = conv(d + "contextual_embedder.0", cfg.mel_channels, C, 3);
    ctx1_ = conv(d + "contextual_embedder.1", C, 2 * C, 3);
    for (int i = 2; i < 7; ++i) ctx_.push_back(attn_block(d + "contextual_embedder." + std::to_string(i), 2 * C, H));
    te0_ = conv(d + "time_embed.0", C, C, 1);
    te2_ = conv(d + "time_embed.2", C, C, 1);

    make_schedule(cfg.diff_trained_steps, space_steps(cfg.diff_trained_steps, cfg.diff_steps), cfg.cond_free_k, sched0_);
    sched0_.id = 0;
    n_resblocks_ = rbi;

    // ---- timestep tables on the device (build_ss_table) in the bind-time arena
    const int NS = sched0_.n, NRB = rbi;
    xpath_ = inp_block;                                          // k = 3, mel_channels -> C: the composition keeps inp_block's shape
    DTTS_REQUIRE(integ1.Cin <= inp_block.CoutP && integ1.CoutP == inp_block.CoutP, "x path: inp_block and integrating_conv do not compose");
    const size_t xw = (size_t)xpath_.KW * xpath_.CinP * xpath_.CoutP;
    persist_.ensure(sizeof(float) * ((size_t)NRB * 2 * C * NS + 3 * (size_t)C * NS + xw + xpath_.CoutP) + sizeof(int) * NS + 4096);
    float* ss_table = persist_.f32((size_t)NRB * 2 * C * NS);
    float* scratch = persist_.f32(3 * (size_t)C * NS);
    int* ts_dev = persist_.i32(NS);
    sched0_.ss_table = ss_table;
    build_ss_table(sched0_, ss_table, scratch, ts_dev, s);

    // ---- the composed x-path conv (compose_xpath_kernel), rebuilt with every (re)bind like the tables above
    {
        float* w = persist_.f32(xw);
        float* b = persist_.f32(xpath_.CoutP);
        const int rows = xpath_.KW * xpath_.CinP;
        hipLaunchKernelGGL(compose_xpath_kernel, dim3(cdiv(xpath_.CoutP, 256), rows + 1), dim3(256), 0, s, inp_block.w, inp_block.b, inp_block.CoutP,
                           integ1.w, integ1.b, integ1.Cin, xpath_.CoutP, rows, w, b);
        DTTS_CHECK_HIP(hipGetLastError());
        xpath_.w = w;
        xpath_.b = b;
    }

    // ---- split-precision (3 x bf16) copies of the trunk's conv weights (conv_x3.h)
    std::vector<PackedConv*> hot = {&xpath_, &integ2_, &out_conv_};
    auto add_layer = [&](DiffLayerW& l) {
        hot.push_back(&l.rb.c1);
        hot.push_back(&l.rb.c2);
        hot.push_back(&l.at.qkv);
        hot.push_back(&l.at.proj);
    };
    for (auto& l : integ_) add_layer(l);
    for (auto& l : layers_) add_layer(l);
    for (auto& r : tail_) { hot.push_back(&r.c1); hot.push_back(&r.c2); }
    // round 4: the 1 x 1 convs of the conditioning encoders' AttentionBlocks too (contextual_embedder: 1536 channels, head dim 96 -
    // fp32 attention between split-precision convs; latent_conditioner: 768 channels, the trunk's block): they run on stage B's stream
    // in front of every request's sampler
    for (auto& b : ctx_) { hot.push_back(&b.qkv); hot.push_back(&b.proj); }
    for (auto& b : latcond_) { hot.push_back(&b.qkv); hot.push_back(&b.proj); }
    size_t total = 0;
    for (PackedConv* pc : hot) {
        DTTS_REQUIRE(pc->Cin == pc->CinP && pc->CoutP % 128 == 0, "trunk conv not eligible for the split-precision path");
        total += (size_t)pc->KW * pc->CinP * pc->CoutP * 4 + 256;
    }
    w3_.ensure(total + 4096);
    for (PackedConv* pc : hot) {
        void* dst = w3_.raw((size_t)pc->KW * pc->CinP * pc->CoutP * 4);
        launch_split_weights(pc->w, pc->KW, pc->CinP, pc->CoutP, dst, s);
        pc->w3 = dst;
    }
}

// floats of the qkv scratch of an AttentionBlock: fp32 rows [B, 3C, T] or, on the split-precision path, the attention's operand
// images (attention.h: AttnPlanes; key tiles padded to 64)
static size_t qkv_floats(int B, int C, int T) {
    const size_t rows = (size_t)3 * B * C * T, planes = (AttnPlanes::bytes(B, C / AttnPlanes::D, T) + 3) / 4;
    return std::max(rows, planes) + 64;
}

bool Model::use_x3() const {
    static const bool on = env_on("DTTS_CONV_X3");
    return on && opt_conv_x3_;
}

// ------------------------------------------------------------------------------ building blocks
void Model::norm_input(const float* x, int C, const float* gamma, const float* beta, int act, bool x3, const TrunkIo& io) {
    const long long bs = (long long)C * io.Ta;
    if (x3) launch_gn_split_planes(x, bs, io.Ta, io.lens, io.T, io.B, C, gn_groups(C), gamma, beta, 1e-5f, nullptr, 0, 0, act, io.xs, io.s);
    else launch_gn_coeffs(x, bs, io.Ta, io.lens, io.T, io.B, C, gn_groups(C), gamma, beta, 1e-5f, nullptr, 0, 0, io.ab, io.s);
}

// AttentionBlock (vqvae/utils/diff_util.py:209-215): y = x + proj(attn(qkv(GN(x))))
void Model::attention_block(const AttnBlockW& w, const float* x, float* y, float* qkv, float* att, const TrunkIo& io) {
    const int C = w.C, D = C / w.H, B = io.B, T = io.T, Ta = io.Ta;
    const long long bs = (long long)C * Ta;
    const bool x3 = io.xs && w.qkv.w3 && w.proj.w3;
    norm_input(x, C, w.gn_g, w.gn_b, ACT_NONE, x3, io);
    ConvParams p = cp(x, C, qkv, 3 * C, B, T, Ta, io.lens);
    p.pro_ab = io.ab;
    const bool planes = x3 && D == AttnPlanes::D;       // (other head dims: fp32 attention, its output is split below)
    DTTS_REQUIRE(!planes || w.bias_tab, "split-precision attention (head dim 48) needs the block's relative-position bias table");
    DTTS_REQUIRE(!io.p1 || planes, "trunk_fp16: the attention has its one-product mode only on the qkv conv's operand images (split-precision path, head dim 48)");
    if (x3) {
        with_planes(p, io.xs, T);
        p.p1 = io.p1;
    }
    if (planes) {            // the qkv conv writes the attention's operand images instead of fp32 rows
        p.qkv_planes = qkv;
        p.qkv_heads = w.H;
        p.qkv_nt64 = AttnPlanes::nt64(T);
        p.qkv_tq = AttnPlanes::tq(T);
        p.qkv_qscale = (1.f / std::sqrt((float)D)) * 1.4426950408889634f;
    }
    run_conv(w.qkv, p, io.s);
    AttnParams a;
    a.qkv = qkv;
    a.bs = 3 * bs;
    a.cs = Ta;
    a.q_off = 0;
    a.k_off = D;
    a.v_off = 2 * D;
    a.head_stride = 3 * D;
    a.out = att;
    a.o_bs = bs;
    a.o_cs = Ta;
    a.lens = io.lens;
    a.T = T;
    a.B = B;
    a.H = w.H;
    a.D = D;
    a.scale = 1.f / std::sqrt((float)D);
    a.bias_tab = w.bias_tab;
    if (planes) a.planes = qkv;
    a.p1 = io.p1;
    if (RowInvariantLaunches::on()) a.ksplit_max = 1;
    // the proj conv's input planes come straight from the attention epilogue; xs still holds the zero halo / tail columns that
    // gn_split_planes wrote for the qkv conv (same B, T, lens), and the qkv conv has consumed the rest
    const bool att_planes = planes && T + 1 < x3_tp(T);
    if (att_planes) {
        a.out_x3 = io.xs;
        a.x3_tp = x3_tp(T);
    }
    launch_flash_attention(a, io.s);
    ConvParams q = cp(att, C, y, C, B, T, Ta, io.lens);
    with_res(q, x, bs, Ta);
    if (x3) {
        if (!att_planes) launch_split_planes(att, bs, Ta, nullptr, ACT_NONE, io.lens, T, B, C, io.xs, io.s);
        with_planes(q, io.xs, T);
        q.p1 = io.p1;
    }
    run_conv(w.proj, q, io.s);
}

// diffusion ResBlock (vqvae/diff_model.py:106-119): y = x + conv3(SiLU(AdaGN(conv1(SiLU(GN(x))))))
void Model::res_block_fwd(const Schedule& sc, const ResBlockW& w, const float* x, float* h1, float* y, int step, const TrunkIo& io) {
    res_block_front(w, x, h1, io);
    res_block_back(sc, w, h1, x, y, step, io);
}

// ... its front, h1 = conv1(SiLU(GN(x))): no timestep enters here
void Model::res_block_front(const ResBlockW& w, const float* x, float* h1, const TrunkIo& io) {
    const int C = cfg.diff_channels;
    const bool x3 = io.xs && w.c1.w3 && w.c2.w3;
    norm_input(x, C, w.gn1_g, w.gn1_b, ACT_SILU, x3, io);
    ConvParams p = cp(x, C, h1, C, io.B, io.T, io.Ta, io.lens);
    p.pro_ab = io.ab;
    p.pro_act = ACT_SILU;
    if (x3) {
        with_planes(p, io.xs, io.T);
        p.p1 = io.p1;
    }
    run_conv(w.c1, p, io.s);
}

// ... and its back, y = x + conv3(SiLU(AdaGN(h1))).  bmod != 0: h1 and x hold bmod samples and sample b of the batch reads sample
// b % bmod of both (the same front under several timesteps: precompute_integrator); bidx [B] = b % bmod on the device, which the exact
// fp32 conv reads h1 through.  The statistics of h1 are still taken inside the norm pass of every sample.
void Model::res_block_back(const Schedule& sc, const ResBlockW& w, const float* h1, const float* x, float* y, int step, const TrunkIo& io,
                           int bmod, const int* bidx) {
    const int C = cfg.diff_channels, B = io.B, T = io.T, Ta = io.Ta, groups = gn_groups(C);
    const long long bs = (long long)C * Ta;
    const bool x3 = io.xs && w.c1.w3 && w.c2.w3;
    const float* ada = sc.ss_table + (size_t)w.index * 2 * C * sc.n + (io.step_idx ? 0 : step);   // step_idx: per-sample steps
    if (x3) launch_gn_split_planes(h1, bs, Ta, io.lens, T, B, C, groups, w.gn2_g, w.gn2_b, 1e-5f, ada, sc.n, 0, ACT_SILU, io.xs, io.s, io.step_idx, bmod);
    else launch_gn_coeffs(h1, bs, Ta, io.lens, T, B, C, groups, w.gn2_g, w.gn2_b, 1e-5f, ada, sc.n, 0, io.ab, io.s, io.step_idx, bmod);
    ConvParams q = cp(h1, C, y, C, B, T, Ta, io.lens);
    q.pro_ab = io.ab;
    q.pro_act = ACT_SILU;
    q.pad = 1;
    if (x3) {
        with_planes(q, io.xs, T);
        q.p1 = io.p1;
    } else if (bmod) {
        DTTS_REQUIRE(bidx, "res_block_back: a shared h1 needs the sample index table");
        q.x_bidx = bidx;
    }
    with_res(q, x, bs, Ta);
    q.res_bmod = bmod;
    run_conv(w.c2, q, io.s);
}

// One batched (cond | uncond) DiffusionTts.forward: x [B,128,T]; cbuf0 [2B,768,T] = (code_emb | uncond broadcast);
// out2 [2B,256,T].  lens2 = device lens repeated twice.
// The unconditional branch of the conditioning_timestep_integrator sees a T-constant input (the broadcast
// unconditioned_embedding), so its output depends only on (timestep, length): it is evaluated once per DISTINCT length in
// the batch instead of once per utterance (identical values, 3 of 16 layers x half the batch less work).
Model::PairPlan Model::plan_pair(const int* lens_host, int B, int T, hipStream_t s) {
    std::vector<int> l2(2 * B), li, um(4 * B), ul;       // um: umap [2B], then xmap [2B]
    for (int b = 0; b < B; ++b) {
        const int len = lens_host ? lens_host[b] : T;
        l2[b] = l2[B + b] = len;
        li.push_back(len);
        um[b] = b;
        um[2 * B + b] = um[3 * B + b] = b;
        int gidx = -1;
        for (size_t k = 0; k < ul.size(); ++k)
            if (ul[k] == len) gidx = (int)k;
        if (gidx < 0) { gidx = (int)ul.size(); ul.push_back(len); }
        um[B + b] = B + gidx;
    }
    for (int v : ul) li.push_back(v);
    PairPlan pl;
    pl.lens_i_host = li;
    pl.Nu = (int)ul.size();
    pl.lens2 = upload_ints(l2.data(), 2 * B, s);
    pl.lens_i = upload_ints(li.data(), (int)li.size(), s);
    pl.umap = upload_ints(um.data(), 4 * B, s);
    pl.xmap = pl.umap + 2 * B;                    // (one table, one copy)
    register_cols(pl.lens2, l2.data(), 2 * B, T, s);
    register_cols(pl.lens_i, li.data(), (int)li.size(), T, s);
    return pl;
}

// One batched (cond | uncond) DiffusionTts.forward.  The two halves are independent until the sampler update, so they run on
// HIP streams of their own (fork, join before returning): the per-launch prologue/epilogue of one chunk's kernels overlaps the matrix
// work of the other's (measured +6..9 % on the conv GEMMs).  DTTS_TWO_STREAMS=0 disables it.
// What a step runs in front of the fork is ONE launch, the split of x_t into planes (none on the exact fp32 kernels).  Each chunk then
// opens with the composed x-path conv (xpath_: inp_block and the x half of integrating_conv, folded at bind time) on the planes of its
// samples' x_t, with the code-path term P = W_integ2 . integrator_output as its residual: stack sample b reads x_t of sample xmap[b] and
// P of sample umap[b] (the unconditional samples share one P per distinct length).  integ: the step's P from precompute_integrator's
// table; without it (diff_step, diff_forward*, a table beyond DTTS_INTEG_MAX_GB) the integrator and one integ2_ launch over its
// B + Nu outputs run here first.
void Model::diff_forward_pair(const Schedule& sc, const float* x, const float* cbuf0, const PairPlan& pl, int B, int T, int step, float* out2,
                              hipStream_t s, const float* integ, const int* umap) {
    const int C = cfg.diff_channels, Ta = T, OC = cfg.diff_out_channels, MC = cfg.mel_channels, Nu = pl.Nu;
    if (!umap || !integ) umap = pl.umap;
    const int *lens2 = pl.lens2, *lens_i = pl.lens_i;
    const long long bs = (long long)C * Ta;
    static const bool env_two = env_on("DTTS_TWO_STREAMS");
    const bool two_streams = env_two && opt_two_streams_;
    const bool x3 = use_x3();
    DTTS_REQUIRE(!opt_trunk_fp16_ || x3, "trunk_fp16 = 1 needs the split-precision kernels (conv_x3 = 1)");

    void* xs0 = nullptr;                                // planes of x_t, read by every chunk's opening conv
    if (x3) {
        xs0 = ws().raw(x3_bytes(B, MC, T));
        launch_split_planes(x, (long long)MC * T, T, nullptr, ACT_NONE, lens2, T, B, MC, xs0, s);
    }
    // Both CFG halves are the same B-sample stack on the same weights: the 2B samples form ONE stack that is cut into NS equal
    // chunks, each a launch sequence on its own HIP stream (fork after the split of x_t, join before returning).  NS = 1: one
    // 2B-sample launch per layer (best per-kernel efficiency: a 768-channel conv is one full wave of workgroups); NS = 2 (default):
    // cond | uncond on two streams - the HBM-bound GroupNorm/split passes and the VALU-bound attention of one chunk run under the
    // matrix work of the other (measured 3.3 % faster end to end than NS = 1 with the fp16-plane kernels); option "cfg_streams".
    static const int env_ns = env_int("DTTS_CFG_STREAMS", 0);
    // default (option 0): 2 chunks from batch 5 up, 1 below (<= 8 samples per layer: a single launch sequence is faster, measured at B = 1, 2, 4)
    int NS = env_ns > 0 ? env_ns : (opt_cfg_streams_ > 0 ? opt_cfg_streams_ : (B <= 4 ? 1 : 2));
    if (!two_streams) NS = 1;
    if (NS > MAX_CFG_STREAMS) NS = MAX_CFG_STREAMS;
    while (NS > 1 && ((2 * B) % NS != 0 || (B % ((2 * B) / NS) != 0 && ((2 * B) / NS) % B != 0))) --NS;
    const int n = 2 * B / NS, Bi = B + Nu;
    for (int k = 1; k < NS; ++k)
        if (!sx_[k - 1]) make_side_stream(&sx_[k - 1]);
    if (NS > 1) ensure_fork_events();
    // conditioning_timestep_integrator (vqvae/diff_model.py:295) on B code embeddings | Nu unconditional inputs, then the code half of
    // integrating_conv (:298) on its outputs: precomputed for all steps before the loop (precompute_integrator), or evaluated here as one
    // (B + Nu)-sample batch
    const float* P = integ;
    if (!integ) {
        float* bufP = ws().f32((size_t)Bi * C * Ta);
        const size_t mark = ws().mark();
        const size_t act = (size_t)Bi * C * Ta;
        float* bufI = ws().f32(act);
        float* tA = ws().f32(act);
        float* tB = ws().f32(act);
        float* qkv = ws().f32(qkv_floats(Bi, C, T));
        TrunkIo io{lens_i, Bi, T, Ta, s, ws().f32((size_t)Bi * C * 2)};
        io.xs = x3 ? ws().raw(x3_bytes(Bi, C, T)) : nullptr;
        const float* in = cbuf0;
        for (int l = 0; l < 3; ++l) {
            res_block_fwd(sc, integ_[l].rb, in, tA, tB, step, io);
            attention_block(integ_[l].at, tB, bufI, qkv, tA, io);
            in = bufI;
        }
        code_half(bufI, bufP, io);
        ws().rewind(mark);
        P = bufP;
    }
    if (NS > 1) {
        DTTS_CHECK_HIP(hipEventRecord(ev_fork_, s));
        for (int k = 1; k < NS; ++k) DTTS_CHECK_HIP(hipStreamWaitEvent(sx_[k - 1], ev_fork_, 0));
    }
    for (int k = 0; k < NS; ++k) {
        hipStream_t st = k ? sx_[k - 1] : s;
        const int b0 = k * n;                          // first sample of the chunk in the 2B stack
        const int* lens = lens2 + b0;
        const size_t act = (size_t)n * C * Ta;
        float* bufA = ws().f32(act);
        float* bufB = ws().f32(act);
        float* bufC = ws().f32(act);
        float* qkv = ws().f32(qkv_floats(n, C, T));
        TrunkIo io{lens, n, T, Ta, st, ws().f32((size_t)n * C * 2)};
        io.xs = x3 ? ws().raw(x3_bytes(n, C, T)) : nullptr;
        // inp_block + integrating_conv (:296-298): the composed x-path conv on x_t, the code-path term as its residual
        ConvParams r = cp(x, MC, T, T, lens, bufB, C, T, Ta, lens, n);
        r.pad = 1;
        r.x_bidx = pl.xmap + b0;                       // x_t of stack sample b: (b0 + b) % B
        with_res(r, P, bs, Ta);
        r.res_bidx = umap + b0;                        // code-path sample of stack sample b (uncond samples share one per length)
        if (x3) with_planes(r, xs0, T);
        run_conv(xpath_, r, st);
        // main stack (:299-309)
        float* cur = bufB;
        float* t1 = bufA;
        float* t2 = bufC;
        for (size_t li = 0; li < layers_.size(); ++li) {   // output back into `cur` (x is dead after the residual add)
            const auto& l = layers_[li];
            io.p1 = opt_trunk_fp16_ && li >= 1;             // layers[0] keeps the three-product kernels (:305-307)
            res_block_fwd(sc, l.rb, cur, t1, t2, step, io);
            attention_block(l.at, t2, cur, qkv, t1, io);
        }
        io.p1 = opt_trunk_fp16_;
        for (size_t ti = 0; ti < tail_.size(); ++ti) {
            res_block_fwd(sc, tail_[ti], cur, t1, t2, step, io);
            std::swap(cur, t2);
        }
        // out: GN, SiLU, conv k3 (:312); three products like the x path
        norm_input(cur, C, out_gn_g_, out_gn_b_, ACT_SILU, x3, io);
        ConvParams o = cp(cur, C, T, Ta, lens, out2 + (size_t)b0 * OC * T, OC, T, T, lens, n);
        o.pro_ab = io.ab;
        o.pro_act = ACT_SILU;
        o.pad = 1;
        if (x3) with_planes(o, io.xs, T);
        run_conv(out_conv_, o, st);
    }
    for (int k = 1; k < NS; ++k) {
        DTTS_CHECK_HIP(hipEventRecord(ev_joinx_[k - 1], sx_[k - 1]));
        DTTS_CHECK_HIP(hipStreamWaitEvent(s, ev_joinx_[k - 1], 0));
    }
}

// the code half of integrating_conv on the integrator's outputs: P = W_integ2 . in (no bias: that is in xpath_), on io's batch and stream
void Model::code_half(const float* in, float* P, const TrunkIo& io) {
    const int C = cfg.diff_channels;
    ConvParams r = cp(in, C, P, C, io.B, io.T, io.Ta, io.lens);
    if (io.xs && integ2_.w3) {
        launch_split_planes(in, (long long)C * io.Ta, io.Ta, nullptr, ACT_NONE, io.lens, io.T, io.B, C, io.xs, io.s);
        with_planes(r, io.xs, io.T);
    }
    run_conv(integ2_, r, io.s);
}

size_t Model::rows_ws_bytes(int B, int C, int T) const {
    const size_t act = (size_t)B * C * T;
    // integrator output (act) + one block's scratch (3 act + qkv + coefficients); planes: x_t, blocks
    return sizeof(float) * (4 * act + qkv_floats(B, C, T) + (size_t)2 * B * C) + x3_bytes(B, cfg.mel_channels, T) + x3_bytes(B, C, T) + 32 * 256;
}

// DiffusionTts.forward (vqvae/diff_model.py:262-322), conditional branch only, every row at its own column of sc: the launch sequence of
// one chunk of diff_forward_pair on the B conditional samples, on s alone, with TrunkIo::step_idx set in the integrator, the stack and
// the tail.
void Model::diff_forward_rows_s(const Schedule& sc, const float* x, const float* code_emb, const int* lens_host, int B, int T,
                                const int* step_of_row, float* out, hipStream_t s) {
    const int C = cfg.diff_channels, Ta = T, OC = cfg.diff_out_channels;
    const long long bs = (long long)C * Ta;
    const size_t act = (size_t)B * C * Ta;
    const bool x3 = use_x3();
    std::vector<int> l(B);
    for (int b = 0; b < B; ++b) l[b] = lens_host ? lens_host[b] : T;
    const int* lens = upload_ints(l.data(), B, s);
    const int* steps = upload_ints(step_of_row, B, s);
    register_cols(lens, l.data(), B, T, s);
    float* bufI = ws().f32(act);
    float* bufA = ws().f32(act);
    float* bufB = ws().f32(act);
    float* bufC = ws().f32(act);
    float* qkv = ws().f32(qkv_floats(B, C, T));
    TrunkIo io{lens, B, T, Ta, s, ws().f32((size_t)B * C * 2)};
    void* xs0 = x3 ? ws().raw(x3_bytes(B, cfg.mel_channels, T)) : nullptr;
    io.xs = x3 ? ws().raw(x3_bytes(B, C, T)) : nullptr;
    io.step_idx = steps;
    // conditioning_timestep_integrator (:295) on the B code embeddings
    const float* in = code_emb;
    for (int li = 0; li < 3; ++li) {
        res_block_fwd(sc, integ_[li].rb, in, bufA, bufB, 0, io);
        attention_block(integ_[li].at, bufB, bufI, qkv, bufA, io);
        in = bufI;
    }
    // integrating_conv, code half (into bufC, free until the first block's c2), then inp_block + the x half as the composed x-path conv
    // (:296-298) with that term as its residual
    code_half(bufI, bufC, io);
    ConvParams r = cp(x, cfg.mel_channels, T, T, lens, bufB, C, T, Ta, lens, B);
    r.pad = 1;
    with_res(r, bufC, bs, Ta);
    if (x3) {
        launch_split_planes(x, r.x_bs, T, nullptr, ACT_NONE, lens, T, B, cfg.mel_channels, xs0, s);
        with_planes(r, xs0, T);
    }
    run_conv(xpath_, r, s);
    // main stack and tail (:299-309), three products throughout
    float* cur = bufB;
    float* t1 = bufA;
    float* t2 = bufC;
    for (const auto& lyr : layers_) {
        res_block_fwd(sc, lyr.rb, cur, t1, t2, 0, io);
        attention_block(lyr.at, t2, cur, qkv, t1, io);
    }
    for (const auto& rb : tail_) {
        res_block_fwd(sc, rb, cur, t1, t2, 0, io);
        std::swap(cur, t2);
    }
    // out: GN, SiLU, conv k3 (:312)
    norm_input(cur, C, out_gn_g_, out_gn_b_, ACT_SILU, x3, io);
    ConvParams o = cp(cur, C, T, Ta, lens, out, OC, T, T, lens, B);
    o.pro_ab = io.ab;
    o.pro_act = ACT_SILU;
    o.pad = 1;
    if (x3) with_planes(o, io.xs, T);
    run_conv(out_conv_, o, s);
    if (sc.used) DTTS_CHECK_HIP(hipEventRecord(sc.used, s));
}

void Model::diff_forward_rows(int sched_id, const float* x, const float* code_emb, const int* lens_host, int B, int T, const int* step_of_row,
                              float* out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(x && code_emb && step_of_row && out && B >= 1 && T >= 1, "diff_forward_rows: x, code_emb, steps, out");
    DTTS_REQUIRE(!opt_trunk_fp16_, "diff_forward_rows runs the three-product trunk only: set trunk_fp16 = 0 for this call");
    const Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_forward_rows runs on an integer-timestep schedule (dtts_diff_schedule)");
    for (int b = 0; b < B; ++b) DTTS_REQUIRE(step_of_row[b] >= 0 && step_of_row[b] < sc.n, "diff_forward_rows: a row's column is outside the schedule");
    ws().ensure(rows_ws_bytes(B, cfg.diff_channels, T) + 8192);
    diff_forward_rows_s(sc, x, code_emb, lens_host, B, T, step_of_row, out, s);
}

// scratch of precompute_integrator: layer 0's shared h1 (Bi samples) + two lanes of Bv samples each
static size_t integ_ws_bytes(int Bi, int Bv, int C, int T) {
    const size_t act = (size_t)Bv * C * T;
    return sizeof(float) * ((size_t)Bi * C * T + 2 * (3 * act + qkv_floats(Bv, C, T) + (size_t)2 * Bv * C)) + 2 * x3_bytes(Bv, C, T) + 32 * 256;
}
static int integ_chunk(int Bi) {     // steps per batched evaluation (~36 samples per launch; DTTS_INTEG_SAMPLES overrides)
    // (batch 1, 12 / 20 / 36 / 52 / 100 samples per launch: diff_sample 122.8 - 126.2 / 123.1 / 123.5 - 124.2 / 123.4 / 123.6 ms - flat within the
    // run-to-run spread, the integrator A/B record under profiles/)
    static const int target = env_int("DTTS_INTEG_SAMPLES", 36);
    return std::max(1, target / Bi);
}

void Model::precompute_integrator(const Schedule& sc, const float* cbuf0, const int* lens_i, const int* lens_i_host, int B, int Nu, int T,
                                  const std::vector<int>& steps, float* integ_all, hipStream_t s, int J_call) {
    const int C = cfg.diff_channels, Bi = B + Nu, J = J_call > 0 ? J_call : integ_chunk(Bi), NS = (int)steps.size();
    const size_t ct = (size_t)C * T, mark = ws().mark();
    const int Bv = J * Bi;
    const bool x3 = use_x3();
    static const bool env_two = env_on("DTTS_TWO_STREAMS");
    const bool two = env_two && opt_two_streams_;
    if (two && !sx_[0]) make_side_stream(&sx_[0]);
    hipStream_t side = sx_[0];
    if (two) ensure_fork_events();
    float* h1 = ws().f32((size_t)Bi * ct);
    // chunks of J steps alternate between the two streams (independent of each other), each with its own scratch
    struct Lane { hipStream_t st; float *bufA, *bufB, *bufC, *qkv, *ab; void* xs; };
    Lane lanes[2];
    for (int q = 0; q < (two ? 2 : 1); ++q) {
        lanes[q].st = q ? side : s;
        lanes[q].bufB = ws().f32((size_t)Bv * ct);
        lanes[q].bufC = ws().f32((size_t)Bv * ct);
        lanes[q].bufA = ws().f32((size_t)Bv * ct);
        lanes[q].qkv = ws().f32(qkv_floats(Bv, C, T));
        lanes[q].ab = ws().f32((size_t)2 * Bv * C);
        lanes[q].xs = x3 ? ws().raw(x3_bytes(Bv, C, T)) : nullptr;
    }
    // Layer 0's front, h1 = c1(SiLU(GN(cbuf0))), sees no timestep (it enters a ResBlock at the second norm): once per request on the
    // Bi inputs, in front of the fork; every chunk's sample j * Bi + b then reads h1 - and cbuf0, the block's residual - of sample b
    {
        TrunkIo io0{lens_i, Bi, T, T, s, lanes[0].ab};
        io0.xs = lanes[0].xs;
        res_block_front(integ_[0].rb, cbuf0, h1, io0);
    }
    if (two) {
        DTTS_CHECK_HIP(hipEventRecord(ev_fork_, s));
        DTTS_CHECK_HIP(hipStreamWaitEvent(side, ev_fork_, 0));
    }
    std::vector<int> lv(Bv), sv(Bv), bv(Bv);
    int ci = 0;
    // profile sampling: both lanes of a chunk pair, or neither - and WHICH pairs rotates from call to call, so that over step_every calls
    // every pair is bracketed exactly once: the bracketed share of this pre-pass is 1 / step_every like the loop's (a fixed choice of
    // pairs 0 and 5 of 7 bracketed 32 % of it, and bench.py's busy share - union x step_every - counted the pre-pass 1.6 x: VERDICT r05)
    const int prof_rot = prof_rot_++;
    for (int k0 = 0; k0 < NS; k0 += J, ++ci) {
        const Lane& L = lanes[two ? (ci & 1) : 0];
        Profiler::gate() = ((ci / 2 + prof_rot) % Profiler::get().step_every) == 0;
        const int jn = std::min(J, NS - k0), nb = jn * Bi;
        for (int j = 0; j < jn; ++j)
            for (int b = 0; b < Bi; ++b) {
                lv[j * Bi + b] = lens_i_host[b];
                sv[j * Bi + b] = steps[k0 + j];
                bv[j * Bi + b] = b;
            }
        const int* dl = upload_ints(lv.data(), nb, L.st);
        const int* ds = upload_ints(sv.data(), nb, L.st);
        const int* db = x3 ? nullptr : upload_ints(bv.data(), nb, L.st);      // (the exact fp32 conv reads the shared h1 through it)
        register_cols(dl, lv.data(), nb, T, L.st);
        float* outp = integ_all + (size_t)k0 * Bi * ct;
        TrunkIo io{dl, nb, T, T, L.st, L.ab};              // (the integrator always takes three products)
        io.xs = L.xs;
        io.step_idx = ds;
        auto dlayer = [&](const DiffLayerW& l, const float* in, float* o) {
            res_block_fwd(sc, l.rb, in, L.bufB, L.bufC, 0, io);
            attention_block(l.at, L.bufC, o, L.qkv, L.bufB, io);
        };
        res_block_back(sc, integ_[0].rb, h1, cbuf0, L.bufC, 0, io, Bi, db);
        attention_block(integ_[0].at, L.bufC, L.bufA, L.qkv, L.bufB, io);
        dlayer(integ_[1], L.bufA, L.bufA);
        dlayer(integ_[2], L.bufA, L.bufA);
        code_half(L.bufA, outp, io);                                       // the table holds P = W_integ2 . integrator output
        register_cols(dl, nullptr, 0, T, L.st);                        // enqueued: forget this chunk's table
    }
    Profiler::gate() = true;
    if (two) {
        DTTS_CHECK_HIP(hipEventRecord(ev_joinx_[0], sx_[0]));
        DTTS_CHECK_HIP(hipStreamWaitEvent(s, ev_joinx_[0], 0));
    }
    ws().rewind(mark);
}

static size_t pair_ws_bytes(int B, int C, int MC, int T) {
    const size_t act = (size_t)B * C * T;
    // the code-path term of a step without the table (B + Nu <= 2B samples) + the scratch of a 2B-sample stack (3 x 2 act + qkv +
    // coefficients + planes): the chunks' together, or in front of them - and given back - the in-step integrator's; planes of x_t
    return sizeof(float) * (2 * act + 2 * (3 * act + qkv_floats(B, C, T) + (size_t)2 * B * C)) + 2 * x3_bytes(B, C, T) + x3_bytes(B, MC, T) + 64 * 256;
}

Model::PairCall Model::begin_pair(const float* code_emb, const int* lens_host, const int* sample_ids_host, int B, int T, hipStream_t s,
                                  size_t extra_bytes, size_t hist_floats, bool defer_uncond) {
    const int C = cfg.diff_channels, OC = cfg.diff_out_channels;
    const size_t half = (size_t)B * C * T;
    ws().ensure(pair_ws_bytes(B, C, cfg.mel_channels, T) + extra_bytes + sizeof(float) * (2 * half + (size_t)2 * B * OC * T + hist_floats) + 8192);
    PairCall pc;
    pc.pl = plan_pair(lens_host, B, T, s);
    pc.sids = sample_ids_host ? upload_ints(sample_ids_host, B, s) : nullptr;
    pc.cbuf0 = ws().f32(2 * half);
    pc.out2 = ws().f32((size_t)2 * B * OC * T);
    pc.hist = hist_floats ? ws().f32(hist_floats) : nullptr;
    if (code_emb) DTTS_CHECK_HIP(hipMemcpyAsync(pc.cbuf0, code_emb, sizeof(float) * half, hipMemcpyDeviceToDevice, s));
    pc.uncond_deferred = defer_uncond;
    for (int h = code_emb ? 1 : 0; h < (defer_uncond ? 1 : 2); ++h)   // the unconditional inputs; without a code embedding the conditional half too
        launch_broadcast_channels(uncond_, h ? pc.pl.Nu : B, C, T, pc.cbuf0 + h * half, (long long)C * T, T, s);
    return pc;
}

// ------------------------------------------------------------------------------ what the sampling entries share
static void check_lens(const int* lens_host, int B, int T) {
    for (int b = 0; lens_host && b < B; ++b) DTTS_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= T, "lens: every length in [1, T]");
}
// May the code-path table of `nst` steps be built?  The terms of all steps are evaluated up front (opt-out: DTTS_INTEG_PRECOMPUTE=0) and
// cost nst * 2B * C * T floats (3 GB at batch 8 x 10 s, 11 GB at batch 4 x 60 s): beyond DTTS_INTEG_MAX_GB (default 24) the integrator
// and the code half run inside every step instead (same values, no table).
static bool integ_table_fits(int nst, int B, int C, int T) {
    static const bool env_pre_on = env_on("DTTS_INTEG_PRECOMPUTE");
    static const double max_gb = []() { const char* v = env_str("DTTS_INTEG_MAX_GB"); return v ? atof(v) : 24.0; }();
    return env_pre_on && (double)(sizeof(float) * (size_t)nst * 2 * B * C * T) <= max_gb * 1073741824.0;
}
static size_t integ_call_bytes(int nst, int B, int C, int T) {        // the table of nst steps + precompute_integrator's scratch (Nu <= B)
    return sizeof(float) * (size_t)nst * 2 * B * C * T + integ_ws_bytes(2 * B, integ_chunk(B + 1) * 2 * B, C, T);
}

// x_T (vqvae/model_24k.py:488): per-sample noise indexed over the sample's own [128, len], so that element order == reference tensor order
void Model::draw_x_T(float* x, const PairCall& pc, const int* lens_host, int B, int T, unsigned long long seed, hipStream_t s) {
    const int MC = cfg.mel_channels;
    const long long xbs = (long long)MC * T;
    DTTS_CHECK_HIP(hipMemsetAsync(x, 0, sizeof(float) * (size_t)B * MC * T, s));
    for (int b = 0; b < B; ++b) {
        const int len = lens_host ? lens_host[b] : T;
        if (len == T) {
            launch_philox_normal(x + (size_t)b * xbs, xbs, MC * T, 1, seed, pc.sids + b, STAGE_DIFF_INIT, 0, 1.f, s);
        } else {
            // compact [128, len] then scatter rows into the padded buffer
            float* tmp = pc.out2;   // free until the first forward
            launch_philox_normal(tmp, 0, MC * len, 1, seed, pc.sids + b, STAGE_DIFF_INIT, 0, 1.f, s);
            DTTS_CHECK_HIP(hipMemcpy2DAsync(x + (size_t)b * xbs, sizeof(float) * T, tmp, sizeof(float) * len, sizeof(float) * len, MC,
                                            hipMemcpyDeviceToDevice, s));
        }
    }
}

// The code-path terms of loop positions [k_first, k_end), carved from ws() and evaluated here: position k is step k of an ascending loop,
// step n - 1 - k of a descending one.  Unpinned, a row's bits follow the width of the launch that made it (split-K), and the whole loop
// evaluates J = integ_chunk steps per launch from position 0: the table then starts at the launch that holds k_first, unneeded steps
// included (at most J - 1), so a loop entered anywhere reads the bits the whole loop reads.  Pinned (RowInvariantLaunches), a row is the
// same bits whatever shares its launch, and the table starts at k_first.
// Unpinned and outside every split regime the unconditional rows come from the per-Model cache where it holds them (DESIGN.md 4.5
// item 4): only the others are evaluated, in the launches the uncached call makes.
Model::CodePathTable Model::code_path_table(const Schedule& sc, const PairCall& pc, int B, int T, int k_first, int k_end, bool descending,
                                            bool pinned, hipStream_t s) {
    const PairPlan& pl = pc.pl;
    const int Bi = B + pl.Nu, J = integ_chunk(Bi);
    CodePathTable t;
    t.k0 = pinned ? k_first : k_first / J * J;
    t.stride = (size_t)Bi * cfg.diff_channels * T;
    std::vector<int> steps(k_end - t.k0);
    for (int k = t.k0; k < k_end; ++k) steps[k - t.k0] = descending ? sc.n - 1 - k : k;
    t.base = ws().f32(steps.size() * t.stride);
    std::optional<RowInvariantLaunches> pin;
    if (pinned) pin.emplace();
    const int C = cfg.diff_channels, Nu = pl.Nu, n = (int)steps.size();
    const size_t ct = (size_t)C * T, slab = sizeof(float) * n * ct;
    auto fill_uncond = [&](int rows) {                                    // begin_pair left the unconditional inputs to this call
        if (pc.uncond_deferred && rows > 0) launch_broadcast_channels(uncond_, rows, C, T, pc.cbuf0 + (size_t)B * ct, (long long)ct, T, s);
    };
    // ---- the unconditional rows from the cache (uncond_cache.h).  Off (budget 0): every row evaluated, nothing counted.  It stands
    // aside - counted - on the exact fp32 kernels, under RowInvariantLaunches (pinned entries neither read nor write it), for a table
    // that does not start at position 0 of a descending loop, and wherever a launch's width picks a summation order (integ_unsplit):
    // a hit must be the miss's bits.  (n * 2B: the per-position index table must fit one upload.)
    bool use = false;
    if (ucache_want_ > 0) {
        use = use_x3() && !pinned && !RowInvariantLaunches::on() && descending && t.k0 == 0 && (size_t)n * 2 * B <= 32768 &&
              integ_unsplit(B, Bi, T, n, J);
        std::lock_guard<std::mutex> lk(ucache_mu_);
        if (use && !ucache_mem_) {                                        // first use: the one allocation
            if (hipMalloc(reinterpret_cast<void**>(&ucache_mem_), ucache_want_) == hipSuccess) {
                ucache_.set_budget(ucache_want_);
            } else {                                                      // no room for the budget: the cache stays off, the call goes on
                (void)hipGetLastError();
                ucache_mem_ = nullptr;
                ucache_want_ = 0;
                use = false;
            }
        }
        if (!use) ucache_.count_bypass();
    }
    if (!use) {
        fill_uncond(Nu);
        precompute_integrator(sc, pc.cbuf0, pl.lens_i, pl.lens_i_host.data(), B, Nu, T, steps, t.base, s);
        return t;
    }
    // (trunk_fp16 is not in the key: the integrator always takes three products)
    UncondKey key;
    key.sched_id = sc.id;
    key.kind = sc.kind;
    key.tmap = sc.tmap;
    key.ftimes = sc.ftimes;
    key.n_pos = n;
    key.T = T;
    const int* ulen = pl.lens_i_host.data() + B;                          // the Nu distinct lengths
    std::vector<int> miss, slot_of(Nu, -1), served_of(Nu, -1), row_of(Nu, -1);   // g -> its slot | its slab behind the evaluated rows | its evaluated row
    std::vector<size_t> off_of(Nu, 0);
    int Nh = 0;
    {
        std::lock_guard<std::mutex> lk(ucache_mu_);
        key.bind_gen = bind_gen_;
        for (int g = 0; g < Nu; ++g) {
            key.len = ulen[g];
            if (const UncondCacheBook::Entry* e = ucache_.lookup(key)) { slot_of[g] = e->slot; off_of[g] = e->off; ++Nh; }
            else { row_of[g] = B + (int)miss.size(); miss.push_back(g); }
        }
        // the served slabs into the block, behind the rows this call evaluates: [n][B + Nm][C][T] | Nh x [n][C][T].  Enqueued under the
        // lock, so no insert can take a slot between its lookup and the `read` record that marks it busy.  A reader first waits for
        // the reader before it: `read`, re-recorded by every reader, then completes only when all of them have.
        const int Bc = B + (int)miss.size();
        float* served = t.base + (size_t)n * Bc * ct;
        for (int g = 0, h = 0; g < Nu; ++g) {
            if (slot_of[g] < 0) continue;
            const UcacheEvents& ev = ucache_ev_[(size_t)slot_of[g]];
            DTTS_CHECK_HIP(hipStreamWaitEvent(s, ev.ready, 0));
            DTTS_CHECK_HIP(hipStreamWaitEvent(s, ev.read, 0));
            DTTS_CHECK_HIP(hipMemcpyAsync(served + (size_t)h * n * ct, ucache_mem_ + off_of[g], slab, hipMemcpyDeviceToDevice, s));
            DTTS_CHECK_HIP(hipEventRecord(ev.read, s));
            served_of[g] = h++;
        }
    }
    const int Nm = (int)miss.size(), Bc = B + Nm;
    if (Nh > 0) {
        // position k reads its rows relative to at(k) = base + k Bc ct: evaluated row r at r, served slab h's row at n Bc + h n + k - k Bc
        t.stride = (size_t)Bc * ct;
        std::vector<int> um((size_t)n * 2 * B);
        for (int k = 0; k < n; ++k)
            for (int b = 0; b < B; ++b) {
                const int g = (int)(std::find(ulen, ulen + Nu, pl.lens_i_host[(size_t)b]) - ulen);    // row b's length among the distinct ones
                um[(size_t)k * 2 * B + b] = b;
                um[(size_t)k * 2 * B + B + b] = row_of[g] >= 0 ? row_of[g] : n * Bc + served_of[g] * n + k - k * Bc;
            }
        t.umap = upload_ints(um.data(), (int)um.size(), s);
        t.umap_stride = 2 * B;
    }
    // the rows left to evaluate: the B conditional ones and the Nm missing lengths, in launches of the CALL's J steps - launch count,
    // chunk boundaries and lane alternation stay those of the uncached call; launches only cover fewer samples
    fill_uncond(Nm);
    if (Nm == Nu) {
        precompute_integrator(sc, pc.cbuf0, pl.lens_i, pl.lens_i_host.data(), B, Nu, T, steps, t.base, s, J);
    } else {
        std::vector<int> li(pl.lens_i_host.begin(), pl.lens_i_host.begin() + B);
        for (int g : miss) li.push_back(ulen[g]);
        const int* dli = upload_ints(li.data(), Bc, s);
        register_cols(dli, li.data(), Bc, T, s);
        precompute_integrator(sc, pc.cbuf0, dli, li.data(), B, Nm, T, steps, t.base, s, J);
        register_cols(dli, nullptr, 0, T, s);
    }
    // after a miss: the new slabs into the cache on this call's stream (rows B + m of every position), `ready` behind each copy
    if (Nm > 0) {
        std::lock_guard<std::mutex> lk(ucache_mu_);
        if (ucache_mem_ && key.bind_gen == bind_gen_)
            for (int m = 0; m < Nm; ++m) {
                key.len = ulen[miss[(size_t)m]];
                const UncondCacheBook::Entry* e = ucache_.insert(key, slab, [this](int slot) { return ucache_slot_busy(slot); });
                if (!e) continue;                                         // larger than the budget, or every candidate slot still busy
                if ((size_t)e->slot >= ucache_ev_.size()) ucache_ev_.resize((size_t)e->slot + 1);
                UcacheEvents& ev = ucache_ev_[(size_t)e->slot];
                if (!ev.ready) {
                    DTTS_CHECK_HIP(hipEventCreateWithFlags(&ev.ready, hipEventDisableTiming));
                    DTTS_CHECK_HIP(hipEventCreateWithFlags(&ev.read, hipEventDisableTiming));
                }
                for (int k = 0; k < n; ++k)
                    DTTS_CHECK_HIP(hipMemcpyAsync(ucache_mem_ + e->off + sizeof(float) * k * ct, t.base + ((size_t)k * Bc + B + m) * ct,
                                                  sizeof(float) * ct, hipMemcpyDeviceToDevice, s));
                DTTS_CHECK_HIP(hipEventRecord(ev.ready, s));
            }
    }
    return t;
}

bool Model::integ_unsplit(int Bi_lo, int Bi_hi, int T, int n_pos, int J) const {
    const bool planes = integ_[0].at.C / integ_[0].at.H == AttnPlanes::D;   // else the fp32 attention, which never splits its keys
    auto conv1 = [&](const PackedConv& c, int nb) { return conv_x3_ksplit(c.CoutP, c.Cin, c.KW, T, nb) == 1; };
    for (int Bi : {Bi_lo, Bi_hi}) {
        if (!conv1(integ_[0].rb.c1, Bi)) return false;                        // layer 0's front: once, on the Bi inputs
        for (int jn : {std::min(J, n_pos), n_pos % J}) {                      // the full launches | the narrower last one
            if (jn == 0) continue;
            const int nb = jn * Bi;
            for (size_t l = 0; l < integ_.size(); ++l) {
                const DiffLayerW& L = integ_[l];
                if (l > 0 && !conv1(L.rb.c1, nb)) return false;
                if (!conv1(L.rb.c2, nb) || !conv1(L.at.qkv, nb) || !conv1(L.at.proj, nb)) return false;
                if (planes && attn_x3b_ksplit(T, L.at.H, nb) != 1) return false;
            }
            if (!conv1(integ2_, nb)) return false;
        }
    }
    return true;
}

bool Model::ucache_slot_busy(int slot) {
    if ((size_t)slot >= ucache_ev_.size() || !ucache_ev_[(size_t)slot].ready) return false;
    for (hipEvent_t e : {ucache_ev_[(size_t)slot].ready, ucache_ev_[(size_t)slot].read}) {
        const hipError_t r = hipEventQuery(e);
        if (r == hipErrorNotReady) return true;
        DTTS_CHECK_HIP(r);
    }
    return false;
}

void Model::ucache_release() {
    std::lock_guard<std::mutex> lk(ucache_mu_);
    for (UcacheEvents& ev : ucache_ev_)
        for (hipEvent_t* e : {&ev.ready, &ev.read})
            if (*e) {
                (void)hipEventSynchronize(*e);
                (void)hipEventDestroy(*e);
                *e = nullptr;
            }
    ucache_ev_.clear();
    if (ucache_mem_) (void)hipFree(ucache_mem_);
    ucache_mem_ = nullptr;
    ucache_.set_budget(0);                                                // (drops the entries; the counters live on)
}

// option "uncond_cache_mb": not a launch path - a change waits for the copies in flight, frees the block, and the next call that can
// use the cache allocates the new budget.  0 = off.
void Model::set_uncond_cache_mb(int mb) {
    DTTS_REQUIRE(mb >= 0, "uncond_cache_mb: megabytes >= 0");
    const size_t want = (size_t)mb << 20;
    if (want == ucache_want_ && (!ucache_mem_ || ucache_.budget() == want)) return;
    ucache_release();
    ucache_want_ = want;
}

UncondCacheStats Model::uncond_cache_stats() {
    std::lock_guard<std::mutex> lk(ucache_mu_);
    return ucache_.stats();
}

// one sampler update on the forward's output pc.out2, x in place: p_sample (0), ddim_sample (1), DPM-Solver++(2M) (2: x0_hist) or
// ddim_reverse_sample (SAMPLER_DDIM_REVERSE: the entries' own, no noise) of step `step`.  pstep: the Philox step field of the noise
// drawn when `noise` is null.
void Model::sampler_update(const Schedule& sc, const PairCall& pc, float* x, int B, int T, int sampler, float eta, int step,
                           unsigned long long seed, int pstep, const float* noise, int denorm, hipStream_t s, float* x0_out, float* x0_hist) {
    const int OC = cfg.diff_out_channels, MC = cfg.mel_channels;
    const long long xbs = (long long)MC * T, obs = (long long)OC * T;
    const int* lens2 = pc.pl.lens2;
    if (sampler == SAMPLER_DDIM_REVERSE)
        launch_ddim_reverse_update(x, xbs, T, pc.out2, obs, T, lens2, T, B, MC, sc.ddim_reverse(step), s, x0_out);
    else if (sampler == 2)
        launch_dpm_update(x, xbs, T, pc.out2, obs, T, lens2, T, B, MC, sc.dpm[step], x0_hist, denorm, s, x0_out);
    else if (sampler == 1)
        launch_ddim_update(x, xbs, T, pc.out2, obs, T, lens2, T, B, MC, sc.ddim(step, eta), seed, pc.sids, pstep, noise, denorm, s, x0_out);
    else
        launch_diff_update(x, xbs, T, pc.out2, obs, T, lens2, T, B, MC, sc.p[step], seed, pc.sids, pstep, noise, denorm, s, x0_out);
}

// The descending sampling loop behind diff_sample_ex, diff_sample_from and diff_inpaint: positions [k_first, k_end), position k at step
// i = n - 1 - k, every step above 0 run `resample` times.  x_init null: x_T is drawn.  The fit decision, the workspace and the table's
// launches are those of a loop over [0, k_end) (code_path_table), so a loop cut in two equals the loop run through; a loop cut short
// (k_end < n) keeps its narrower last launch.  Evaluation e (counted from k_first) indexes the noise and trajectory arrays and the
// profiler's sampling; repeat r of step i draws on the Philox step field i + r * n, so repeat 0 is the plain loop's key.
void Model::sample_loop(Schedule& sc, const SampleLoop& c, const float* code_emb, const int* lens_host, int B, int T, unsigned long long seed,
                        const int* sample_ids_host, const float* x_init, float* x, hipStream_t s) {
    const int C = cfg.diff_channels, MC = cfg.mel_channels;
    const size_t plane = (size_t)B * MC * T;
    const bool fits = integ_table_fits(c.k_end, B, C, T);
    // (with a table and the unconditional cache on, code_path_table fills the unconditional inputs: only the rows it evaluates)
    const PairCall pc = begin_pair(code_emb, lens_host, sample_ids_host, B, T, s, fits ? integ_call_bytes(c.k_end, B, C, T) : 0,
                                   c.sampler == 2 ? plane : 0,                // DPM-Solver++(2M): the previous step's x0
                                   fits && ucache_want_ > 0 && use_x3() && !RowInvariantLaunches::on());
    if (!x_init)
        draw_x_T(x, pc, lens_host, B, T, seed, s);
    else if (x != x_init)
        DTTS_CHECK_HIP(hipMemcpyAsync(x, x_init, sizeof(float) * plane, hipMemcpyDeviceToDevice, s));
    const CodePathTable tab = fits ? code_path_table(sc, pc, B, T, c.k_first, c.k_end, true, false, s) : CodePathTable{};
    const size_t mark = ws().mark();
    size_t e = 0;
    for (int k = c.k_first; k < c.k_end; ++k) {
        const int i = sc.n - 1 - k, reps = i == 0 ? 1 : c.resample;
        for (int r = 0; r < reps; ++r, ++e) {
            Profiler::gate() = (e % Profiler::get().step_every) == 0;
            ws().rewind(mark);                              // the forward's scratch is re-carved every evaluation
            diff_forward_pair(sc, x, pc.cbuf0, pc.pl, B, T, i, pc.out2, s, tab.at(k), tab.umap_at(k));
            const int pstep = i + r * sc.n;
            sampler_update(sc, pc, x, B, T, c.sampler, c.eta, i, seed, pstep, c.step_noise ? c.step_noise + e * plane : nullptr,
                           (c.denorm && k == c.k_end - 1) ? 1 : 0, s, nullptr, pc.hist);
            if (c.known)    // the kept frames back at level i - 1 and, before another repeat, x one forward step up again (diff_inpaint.h)
                launch_inpaint_blend(x, c.known, c.keep, pc.pl.lens2, T, B, MC, sc.inpaint(i), i == 0 ? 1 : 0, r < reps - 1 ? 1 : 0, seed, pc.sids,
                                     pstep, c.known_noise ? c.known_noise + e * plane : nullptr, c.renoise ? c.renoise + e * plane : nullptr, s);
            if (c.x_traj) DTTS_CHECK_HIP(hipMemcpyAsync(c.x_traj + e * plane, x, sizeof(float) * plane, hipMemcpyDeviceToDevice, s));
        }
    }
    Profiler::gate() = true;
    if (sc.used) DTTS_CHECK_HIP(hipEventRecord(sc.used, s));
}

// What the single-step entries share: the call's set-up, the forward at `step` - with pinned_table behind a one-step code-path table
// under RowInvariantLaunches, which is diff_invert's step bit for bit - then the caller's update on pc.out2
template <class Update>
void Model::single_step(Schedule& sc, const float* x, const float* code_emb, const int* lens_host, const int* sample_ids_host, int B, int T,
                        int step, bool pinned_table, hipStream_t s, Update&& update) {
    const PairCall pc = begin_pair(code_emb, lens_host, sample_ids_host, B, T, s, pinned_table ? integ_call_bytes(1, B, cfg.diff_channels, T) : 0);
    const CodePathTable tab = pinned_table ? code_path_table(sc, pc, B, T, step, step + 1, false, true, s) : CodePathTable{};
    diff_forward_pair(sc, x, pc.cbuf0, pc.pl, B, T, step, pc.out2, s, tab.at(step));
    update(pc);
    if (sc.used) DTTS_CHECK_HIP(hipEventRecord(sc.used, s));
}

// ------------------------------------------------------------------------------ stage entry points
void Model::diff_forward(const float* x, const float* code_emb, const int* lens_host, int B, int T, int step, int cond_free,
                         float* out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(step >= 0 && step < sched0_.n, "step out of range");
    diff_forward_s(sched0_, x, code_emb, lens_host, B, T, step, cond_free, out, s);
}

void Model::diff_forward_s(Schedule& sc, const float* x, const float* code_emb, const int* lens_host, int B, int T, int step, int cond_free,
                           float* out, hipStream_t s) {
    const int OC = cfg.diff_out_channels;
    const PairCall pc = begin_pair(code_emb, lens_host, nullptr, B, T, s);
    const PairPlan& pl = pc.pl;
    diff_forward_pair(sc, x, pc.cbuf0, pl, B, T, step, pc.out2, s);
    const float* src = pc.out2 + (cond_free ? (size_t)B * OC * T : 0);
    DTTS_CHECK_HIP(hipMemcpyAsync(out, src, sizeof(float) * (size_t)B * OC * T, hipMemcpyDeviceToDevice, s));
}

void Model::diff_forward_t(const float* x, const float* code_emb, const int* lens_host, int B, int T, int timestep, int cond_free,
                           float* out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(timestep >= 0 && timestep < cfg.diff_trained_steps, "timestep out of [0, diff_trained_steps)");
    const auto it = std::lower_bound(sched0_.tmap.begin(), sched0_.tmap.end(), timestep);
    if (it != sched0_.tmap.end() && *it == timestep) {               // a default-schedule timestep: its step of that table
        diff_forward_s(sched0_, x, code_emb, lens_host, B, T, (int)(it - sched0_.tmap.begin()), cond_free, out, s);
        return;
    }
    Schedule& sc = schedule(diff_schedule(&timestep, 1, s));          // a one-step schedule: only its AdaGN table is used
    diff_forward_s(sc, x, code_emb, lens_host, B, T, 0, cond_free, out, s);
    DTTS_CHECK_HIP(hipEventRecord(sc.used, s));
}

void Model::diff_forward_tf(const float* x, const float* code_emb, const int* lens_host, int B, int T, float timestep, int cond_free,
                            float* out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(std::isfinite(timestep) && timestep >= 0.f && timestep < (float)cfg.diff_trained_steps,
                 "timestep out of [0, diff_trained_steps)");
    if (timestep == std::floor(timestep)) {                           // an integer time: diff_forward_t's route, bit for bit
        diff_forward_t(x, code_emb, lens_host, B, T, (int)timestep, cond_free, out, s);
        return;
    }
    auto key = std::make_unique<Schedule>();                          // a one-column fractional schedule: only its AdaGN table is used
    key->kind = 2;
    key->n = 1;
    key->ftimes = {timestep};
    Schedule& sc = schedule(cache_schedule(std::move(key), s));
    diff_forward_s(sc, x, code_emb, lens_host, B, T, 0, cond_free, out, s);
    DTTS_CHECK_HIP(hipEventRecord(sc.used, s));
}

void Model::diff_sample(const float* code_emb, const int* lens_host, int B, int T, unsigned long long seed,
                        const int* sample_ids_host, int n_steps, const float* x_init, const float* step_noise, float* mel_out,
                        int denorm, hipStream_t s) {
    diff_sample_ex(0, 0, 0.f, code_emb, lens_host, B, T, seed, sample_ids_host, n_steps, x_init, step_noise, mel_out, denorm, s);
}

// the first n_steps steps of the schedule from x_init, or from a drawn x_T: sample_loop over positions [0, n_steps)
void Model::diff_sample_ex(int sched_id, int sampler, float eta, const float* code_emb, const int* lens_host, int B, int T,
                           unsigned long long seed, const int* sample_ids_host, int n_steps, const float* x_init, const float* step_noise,
                           float* mel_out, int denorm, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(sampler == 0 || sampler == 1 || sampler == 2, "sampler: 0 (p), 1 (ddim) or 2 (dpmsolver++)");
    DTTS_REQUIRE(eta >= 0.f, "eta must be >= 0");
    Schedule& sc = schedule(sched_id);
    const bool dpm = sampler == 2;
    DTTS_REQUIRE(dpm == (sc.kind == 1), dpm ? "sampler 2 (dpmsolver++) runs on a DPM schedule (dtts_diff_schedule_dpm)"
                                            : "samplers 0 / 1 run on an integer-timestep schedule (dtts_diff_schedule)");
    DTTS_REQUIRE(!dpm || (eta == 0.f && !step_noise), "dpmsolver++ draws no noise: eta must be 0 and step_noise NULL");
    SampleLoop c;
    c.sampler = sampler;
    c.eta = eta;
    c.k_end = (n_steps <= 0 || n_steps > sc.n) ? sc.n : n_steps;
    c.step_noise = step_noise;
    c.denorm = denorm;
    sample_loop(sc, c, code_emb, lens_host, B, T, seed, sample_ids_host, x_init, mel_out, s);
}

// GaussianDiffusion.p_sample (vqvae/utils/diffusion.py:445-485) at one sampling step, x in place
void Model::diff_p_sample(float* x, const float* code_emb, const int* lens_host, int B, int T, int step, unsigned long long seed,
                          const int* sample_ids_host, const float* noise, float* x0_out, hipStream_t s) {
    diff_step(0, 0, 0.f, x, code_emb, lens_host, B, T, step, seed, sample_ids_host, noise, x0_out, s);
}

// one p_sample (vqvae/utils/diffusion.py:445-485) or ddim_sample (:744-783) of schedule `sched_id` at spaced step `step`, x in place
void Model::diff_step(int sched_id, int sampler, float eta, float* x, const float* code_emb, const int* lens_host, int B, int T, int step,
                      unsigned long long seed, const int* sample_ids_host, const float* noise, float* x0_out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(sampler == 0 || sampler == 1, "sampler: 0 (p) or 1 (ddim)");
    DTTS_REQUIRE(eta >= 0.f, "eta must be >= 0");
    Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_step runs on an integer-timestep schedule (DPM-Solver++: diff_step_dpm)");
    DTTS_REQUIRE(step >= 0 && step < sc.n, "step out of range");
    DTTS_REQUIRE(sample_ids_host, "sample_ids");
    single_step(sc, x, code_emb, lens_host, sample_ids_host, B, T, step, false, s, [&](const PairCall& pc) {
        sampler_update(sc, pc, x, B, T, sampler, eta, step, seed, step, noise, 0, s, x0_out);
    });
}

// ---- DDIM inversion, partial-depth sampling, p_mean_variance
// GaussianDiffusion.ddim_reverse_sample (vqvae/utils/diffusion.py:785-817) for t = 0 .. depth - 1.  The code-path terms are evaluated for
// exactly those steps, in that order, under RowInvariantLaunches (code_path_table, pinned), so diff_reverse_step - a table of one step -
// computes this loop's step bit for bit.  A table beyond DTTS_INTEG_MAX_GB is built one step at a time inside the loop (same values).
void Model::diff_invert(int sched_id, const float* code_emb, const int* lens_host, int B, int T, const float* x_start, int depth,
                        float* x_out, float* x_traj, float* x0_traj, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(code_emb && x_start && x_out && B >= 1 && T >= 1, "diff_invert: code_emb, x_start, x_out");
    Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_invert runs on an integer-timestep schedule (dtts_diff_schedule)");
    DTTS_REQUIRE(depth >= 1 && depth <= sc.n, "diff_invert: depth out of [1, steps of the schedule]");
    check_lens(lens_host, B, T);
    const int C = cfg.diff_channels, MC = cfg.mel_channels;
    const bool fits = integ_table_fits(depth, B, C, T);
    const PairCall pc = begin_pair(code_emb, lens_host, nullptr, B, T, s, integ_call_bytes(fits ? depth : 1, B, C, T));
    const PairPlan& pl = pc.pl;
    const size_t plane = (size_t)B * MC * T;
    float* x = x_out;
    if (x != x_start) DTTS_CHECK_HIP(hipMemcpyAsync(x, x_start, sizeof(float) * plane, hipMemcpyDeviceToDevice, s));
    // without the table: one slot (stride 0), refilled in front of every step
    const CodePathTable tab = fits ? code_path_table(sc, pc, B, T, 0, depth, false, true, s)
                                   : CodePathTable{ws().f32((size_t)(B + pl.Nu) * C * T), 0, 0};
    const size_t mark = ws().mark();
    for (int i = 0; i < depth; ++i) {
        Profiler::gate() = (i % Profiler::get().step_every) == 0;
        ws().rewind(mark);
        if (!fits) {
            RowInvariantLaunches pin;
            precompute_integrator(sc, pc.cbuf0, pl.lens_i, pl.lens_i_host.data(), B, pl.Nu, T, std::vector<int>{i}, tab.base, s);
        }
        diff_forward_pair(sc, x, pc.cbuf0, pl, B, T, i, pc.out2, s, tab.at(i));
        sampler_update(sc, pc, x, B, T, SAMPLER_DDIM_REVERSE, 0.f, i, 0, i, nullptr, 0, s, x0_traj ? x0_traj + (size_t)i * plane : nullptr);
        if (x_traj) DTTS_CHECK_HIP(hipMemcpyAsync(x_traj + (size_t)i * plane, x, sizeof(float) * plane, hipMemcpyDeviceToDevice, s));
    }
    Profiler::gate() = true;
    if (sc.used) DTTS_CHECK_HIP(hipEventRecord(sc.used, s));
}

// one ddim_reverse_sample at spaced step `step`: diff_invert's step (a one-step table under RowInvariantLaunches), x in place
void Model::diff_reverse_step(int sched_id, float* x, const float* code_emb, const int* lens_host, int B, int T, int step, float* x0_out,
                              hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(x && code_emb && B >= 1 && T >= 1, "diff_reverse_step: x, code_emb");
    Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_reverse_step runs on an integer-timestep schedule (dtts_diff_schedule)");
    DTTS_REQUIRE(step >= 0 && step < sc.n, "step out of range");
    check_lens(lens_host, B, T);
    single_step(sc, x, code_emb, lens_host, nullptr, B, T, step, true, s, [&](const PairCall& pc) {
        sampler_update(sc, pc, x, B, T, SAMPLER_DDIM_REVERSE, 0.f, step, 0, step, nullptr, 0, s, x0_out);
    });
}

// GaussianDiffusion.p_mean_variance (vqvae/utils/diffusion.py:284-386) at spaced step `step`: diff_step's forward, nothing sampled
void Model::diff_mean_variance(int sched_id, const float* x, const float* code_emb, const int* lens_host, int B, int T, int step,
                               float* mean, float* variance, float* log_variance, float* pred_xstart, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(x && code_emb && mean && variance && log_variance && pred_xstart && B >= 1 && T >= 1,
                 "diff_mean_variance: x, code_emb and the four outputs");
    Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_mean_variance runs on an integer-timestep schedule (dtts_diff_schedule)");
    DTTS_REQUIRE(step >= 0 && step < sc.n, "step out of range");
    check_lens(lens_host, B, T);
    const int OC = cfg.diff_out_channels, MC = cfg.mel_channels;
    single_step(sc, x, code_emb, lens_host, nullptr, B, T, step, false, s, [&](const PairCall& pc) {
        launch_diff_mean_variance(x, (long long)MC * T, T, pc.out2, (long long)OC * T, T, pc.pl.lens2, T, B, MC, sc.p[step], mean, variance,
                                  log_variance, pred_xstart, s);
    });
}

// diff_sample_ex entered at step `first_step`: x_init is x at that level, steps first_step .. 0 run, Philox noise keyed by the step index
// as in the whole loop: sample_loop over positions [n - 1 - first_step, n), whose table makes a loop cut in two equal the loop run through
void Model::diff_sample_from(int sched_id, int sampler, float eta, int first_step, const float* code_emb, const int* lens_host, int B, int T,
                             unsigned long long seed, const int* sample_ids_host, const float* x_init, const float* step_noise,
                             float* mel_out, int denorm, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(sampler == 0 || sampler == 1, "diff_sample_from: sampler 0 (p) or 1 (ddim)");
    DTTS_REQUIRE(eta >= 0.f, "eta must be >= 0");
    DTTS_REQUIRE(code_emb && x_init && mel_out && sample_ids_host && B >= 1 && T >= 1, "diff_sample_from: code_emb, x_init, mel_out, sample_ids");
    Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_sample_from runs on an integer-timestep schedule (dtts_diff_schedule)");
    DTTS_REQUIRE(first_step >= 0 && first_step < sc.n, "diff_sample_from: first_step out of [0, steps of the schedule)");
    check_lens(lens_host, B, T);
    SampleLoop c;
    c.sampler = sampler;
    c.eta = eta;
    c.k_first = sc.n - 1 - first_step;
    c.k_end = sc.n;
    c.step_noise = step_noise;
    c.denorm = denorm;
    sample_loop(sc, c, code_emb, lens_host, B, T, seed, sample_ids_host, x_init, mel_out, s);
}

// ---- mel inpainting (RePaint, Lugmayr et al. 2022): diff_sample_from with the kept frames overwritten after every update
// Step i, repeat r of U: the unchanged sampler update takes x from level i to i - 1, the blend (diff_inpaint.h) overwrites the kept
// frames with `known` at level i - 1 and, for r < U - 1, takes x one forward step back up to level i.  Step 0 runs once.  All three
// noise streams carry the Philox step field i + r * N: the update kernels' `step` argument feeds only the key, so repeat 0 of
// STAGE_DIFF_STEP is the plain loop's key and a call with nothing kept and U = 1 is diff_sample_from bit for bit: both are sample_loop,
// whose table every repeat of a step reads again.
void Model::diff_inpaint(int sched_id, int sampler, float eta, int first_step, int resample, const float* code_emb, const int* lens_host,
                         int B, int T, unsigned long long seed, const int* sample_ids_host, const float* x_init, const float* known,
                         const unsigned char* keep, const float* step_noise, const float* known_noise, const float* renoise, float* x_out,
                         float* x_traj, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(sampler == 0 || sampler == 1, "diff_inpaint: sampler 0 (p) or 1 (ddim); a multistep solver's history does not survive the overwrite");
    DTTS_REQUIRE(eta >= 0.f, "eta must be >= 0");
    DTTS_REQUIRE(resample >= 1 && resample <= 32, "diff_inpaint: resample out of [1, 32]");
    DTTS_REQUIRE(known && keep, "diff_inpaint: known and keep");
    DTTS_REQUIRE(code_emb && x_out && sample_ids_host && B >= 1 && T >= 1, "diff_inpaint: code_emb, x_out, sample_ids");
    Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 0, "diff_inpaint runs on an integer-timestep schedule (dtts_diff_schedule)");
    DTTS_REQUIRE(first_step >= 0 && first_step < sc.n, "diff_inpaint: first_step out of [0, steps of the schedule)");
    DTTS_REQUIRE(x_init || first_step == sc.n - 1, "diff_inpaint: x_init is required below the top of the schedule");
    check_lens(lens_host, B, T);
    SampleLoop c;
    c.sampler = sampler;
    c.eta = eta;
    c.k_first = sc.n - 1 - first_step;
    c.k_end = sc.n;
    c.resample = resample;
    c.known = known;
    c.keep = keep;
    c.known_noise = known_noise;
    c.renoise = renoise;
    c.step_noise = step_noise;
    c.x_traj = x_traj;
    sample_loop(sc, c, code_emb, lens_host, B, T, seed, sample_ids_host, x_init, x_out, s);
}

void Model::op_inpaint_blend(float* x, const float* known, const unsigned char* keep, const int* lens_host, int B, int C, int T,
                             InpaintCoefs k, int step0, int renoise, unsigned long long seed, const int* sample_ids_host, int pstep,
                             const float* known_noise, const float* renoise_noise, hipStream_t s) {
    DTTS_REQUIRE(x && known && keep && B >= 1 && C >= 1 && T >= 1, "op_inpaint_blend: x, known, keep");
    check_lens(lens_host, B, T);
    const int* dl = lens_host ? upload_ints(lens_host, B, s) : nullptr;
    const int* sids = sample_ids_host ? upload_ints(sample_ids_host, B, s) : nullptr;
    launch_inpaint_blend(x, known, keep, dl, T, B, C, k, step0, renoise, seed, sids, pstep, known_noise, renoise_noise, s);
}

// one DPM-Solver++(2M) step (vqvae/utils/dpm_solver.py:1176-1208 per step) of DPM schedule `sched_id` at step index `step`, x in place
void Model::diff_step_dpm(int sched_id, float* x, float* x0_hist, const float* code_emb, const int* lens_host, int B, int T, int step,
                          float* x0_out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    Schedule& sc = schedule(sched_id);
    DTTS_REQUIRE(sc.kind == 1, "diff_step_dpm runs on a DPM schedule (dtts_diff_schedule_dpm)");
    DTTS_REQUIRE(step >= 0 && step < sc.n, "step out of range");
    DTTS_REQUIRE(x && x0_hist && code_emb, "x, x0_hist, code_emb");
    single_step(sc, x, code_emb, lens_host, nullptr, B, T, step, false, s, [&](const PairCall& pc) {
        sampler_update(sc, pc, x, B, T, 2, 0.f, step, 0, step, nullptr, 0, s, x0_out, x0_hist);
    });
}

void Model::diff_conditioning(const float* refer, const int* lens_host, int B, int Tmax, float* cond_out, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    const int C = cfg.diff_channels, C2 = 2 * C;
    const int T1 = (Tmax - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1;
    std::vector<int> l0(B), l1(B), l2(B);
    for (int b = 0; b < B; ++b) {
        l0[b] = lens_host ? lens_host[b] : Tmax;
        l1[b] = (l0[b] - 1) / 2 + 1;
        l2[b] = (l1[b] - 1) / 2 + 1;
    }
    const size_t act = (size_t)B * C2 * T2;
    const bool x3c = use_x3() && !ctx_.empty() && ctx_[0].qkv.w3;
    ws().ensure(sizeof(float) * ((size_t)B * C * T1 + 3 * act + qkv_floats(B, C2, T2) + (size_t)2 * B * C2) + (x3c ? x3_bytes(B, C2, T2) : 0) + 8192);
    const int* d0 = upload_ints(l0.data(), B, s);
    const int* d1 = upload_ints(l1.data(), B, s);
    const int* d2 = upload_ints(l2.data(), B, s);
    float* h1 = ws().f32((size_t)B * C * T1);
    float* a = ws().f32(act);
    float* bb = ws().f32(act);
    float* att = ws().f32(act);
    float* qkv = ws().f32(qkv_floats(B, C2, T2));
    TrunkIo io{d2, B, T2, T2, s, ws().f32((size_t)2 * B * C2)};
    io.xs = x3c ? ws().raw(x3_bytes(B, C2, T2)) : nullptr;
    ConvParams p = cp(refer, cfg.mel_channels, Tmax, Tmax, d0, h1, C, T1, T1, d1, B);
    p.stride = 2;
    p.pad = 1;
    run_conv(ctx0_, p, s);
    ConvParams q = cp(h1, C, T1, T1, d1, a, C2, T2, T2, d2, B);
    q.stride = 2;
    q.pad = 1;
    run_conv(ctx1_, q, s);
    float* cur = a;
    float* nxt = bb;
    for (auto& blk : ctx_) {
        attention_block(blk, cur, nxt, qkv, att, io);
        std::swap(cur, nxt);
    }
    launch_mean_time(cur, (long long)C2 * T2, T2, d2, T2, B, C2, cond_out, s);
}

void Model::diff_timestep_independent(const float* latent_cm, const int* lens_n_host, int B, int nmax, const float* cond,
                                      float* code_emb, hipStream_t s) {
    diff_timestep_independent_ex(latent_cm, lens_n_host, B, nmax, cond, nullptr, nullptr, 0, code_emb, s);
}

void Model::diff_timestep_independent_ex(const float* latent_cm, const int* lens_n_host, int B, int nmax, const float* cond,
                                         const int* frames_host, const int* durations_host, int Tmax, float* code_emb, hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(frames_host || !durations_host, "durations need frames");
    if (frames_host) check_frames(lens_n_host, frames_host, durations_host, B, nmax, Tmax);      // refusals before any launch
    const int C = cfg.diff_channels;
    const size_t act = (size_t)B * C * nmax;
    const bool x3l = use_x3() && !latcond_.empty() && latcond_[0].qkv.w3;
    ws().ensure(sizeof(float) * (3 * act + qkv_floats(B, C, nmax) + (size_t)2 * B * C) + (x3l ? x3_bytes(B, C, nmax) : 0) + 8192 +
                (frames_host ? sizeof(int) * (size_t)B * Tmax + 256 : 0));
    std::vector<int> ln(B);
    for (int b = 0; b < B; ++b) ln[b] = lens_n_host ? lens_n_host[b] : nmax;
    const int* dl = upload_ints(ln.data(), B, s);
    float* a = ws().f32(act);
    float* bb = ws().f32(act);
    float* att = ws().f32(act);
    float* qkv = ws().f32(qkv_floats(B, C, nmax));
    TrunkIo io{dl, B, nmax, nmax, s, ws().f32((size_t)2 * B * C)};
    io.xs = x3l ? ws().raw(x3_bytes(B, C, nmax)) : nullptr;
    const long long bs = (long long)C * nmax;
    ConvParams p = cp(latent_cm, C, a, C, B, nmax, nmax, dl);
    p.pad = 1;
    run_conv(latcond0_, p, s);
    float* cur = a;
    float* nxt = bb;
    for (auto& blk : latcond_) {
        attention_block(blk, cur, nxt, qkv, att, io);
        std::swap(cur, nxt);
    }
    // code_norm(code_emb) * (1 + cond_scale) + cond_shift  (vqvae/diff_model.py:236, 242), then nearest x4 (:252)
    launch_gn_coeffs(cur, bs, nmax, dl, nmax, B, C, gn_groups(C), code_gn_g_, code_gn_b_, 1e-5f, cond, 1, 2 * C, io.ab, s);
    if (!frames_host) {
        launch_affine_apply(cur, bs, nmax, io.ab, dl, nmax, B, C, 4, ACT_NONE, code_emb, (long long)C * 4 * nmax, 4 * nmax, s);
        return;
    }
    // ... or F.interpolate(size=T_b, mode='nearest') / repeat_interleave of the plan, through the row maps (frame_map.hip)
    const int* df = upload_ints(frames_host, B, s);
    int* map = ws().i32((size_t)B * Tmax);
    frame_map_device(dl, df, durations_host, B, nmax, Tmax, map, s);
    affine_gather(cur, bs, nmax, io.ab, df, map, Tmax, B, C, code_emb, s);
}

void Model::op_attention_block(const char* prefix, const float* x, const int* lens_host, int B, int C, int T, float* y,
                               hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    AttnBlockW w = attn_block(prefix, C, cfg.diff_heads);
    const size_t act = (size_t)B * C * T;
    ws().ensure(sizeof(float) * (act + qkv_floats(B, C, T) + (size_t)2 * B * C) + x3_bytes(B, C, T) + 8192);
    std::vector<int> l(B);
    for (int b = 0; b < B; ++b) l[b] = lens_host ? lens_host[b] : T;
    const int* dl = upload_ints(l.data(), B, s);
    float* qkv = ws().f32(qkv_floats(B, C, T));
    float* att = ws().f32(act);
    TrunkIo io{dl, B, T, T, s, ws().f32((size_t)2 * B * C)};
    // the trunk's blocks take the split-precision path exactly as inside diff_forward; io.p1: the layer-index rule of the trunk's
    // fp16 mode, as inside diff_forward
    for (auto* grp : {&integ_, &layers_})
        for (size_t i = 0; i < grp->size(); ++i)
            if ((*grp)[i].at.qkv.w == w.qkv.w) {
                w = (*grp)[i].at;
                io.p1 = opt_trunk_fp16_ && grp == &layers_ && i >= 1;
            }
    io.xs = (use_x3() && w.qkv.w3) ? ws().raw(x3_bytes(B, C, T)) : nullptr;
    attention_block(w, x, y, qkv, att, io);
}

void Model::op_resblock(const char* prefix, const float* x, const int* lens_host, int B, int T, int step, float* y,
                        hipStream_t s) {
    DTTS_REQUIRE(bound_, "weights not bound");
    DTTS_REQUIRE(step >= 0 && step < sched0_.n, "step out of range");
    const int C = cfg.diff_channels;
    const ResBlockW* found = nullptr;
    const std::string pf(prefix);
    bool p1 = false;                                    // the layer-index rule of the trunk's fp16 mode, as inside diff_forward
    auto check = [&](const ResBlockW& r, const std::string& name, bool covered) {
        if (name == pf) { found = &r; p1 = opt_trunk_fp16_ && covered; }
    };
    for (size_t i = 0; i < integ_.size(); ++i) check(integ_[i].rb, "diffusion.conditioning_timestep_integrator." + std::to_string(i) + ".resblk", false);
    for (size_t i = 0; i < layers_.size(); ++i) check(layers_[i].rb, "diffusion.layers." + std::to_string(i) + ".resblk", i >= 1);
    for (size_t i = 0; i < tail_.size(); ++i) check(tail_[i], "diffusion.layers." + std::to_string(layers_.size() + i), true);
    DTTS_REQUIRE(found, "unknown resblock prefix");
    const size_t act = (size_t)B * C * T;
    ws().ensure(sizeof(float) * (act + (size_t)2 * B * C) + x3_bytes(B, C, T) + 8192);
    std::vector<int> l(B);
    for (int b = 0; b < B; ++b) l[b] = lens_host ? lens_host[b] : T;
    const int* dl = upload_ints(l.data(), B, s);
    float* h1 = ws().f32(act);
    TrunkIo io{dl, B, T, T, s, ws().f32((size_t)2 * B * C)};
    io.xs = use_x3() ? ws().raw(x3_bytes(B, C, T)) : nullptr;
    io.p1 = p1;
    res_block_fwd(sched0_, *found, x, h1, y, step, io);
}

}  // namespace dtts
