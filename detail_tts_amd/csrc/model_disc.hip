// The flow-VAE stage's losses on the device: MultiPeriodDiscriminator.forward (vqvae/model_24k.py:298-431), the three GAN loss functions
// (vqvae/modules/losses.py:4-40), spec_to_mel_torch (vqvae/utils/data_utils.py:89-102) and the stage call that returns what
// train.py:259-322 logs.  Forward values only.  Kernels: disc.h; the dense convs are conv_gemm.h launches.
#include "model.h"

namespace dtts {

static const char* kNoDisc = "discriminators.0.convs.0.weight is not bound (bind the checkpoint's 'D' entry first: MultiPeriodDiscriminator / load_discriminator)";
static const int kPeriods[5] = {2, 3, 5, 7, 11};
static const int kSCh[6] = {16, 64, 256, 1024, 1024, 1024};          // DiscriminatorS convs.0 .. 5 output channels
static const int kSGroups[5] = {1, 4, 16, 64, 256};
static const int kPCh[5] = {32, 128, 512, 1024, 1024};               // DiscriminatorP convs.0 .. 4

static long long up16(long long n) { return (n + 15) / 16 * 16; }

DiscLayout disc_layout(int N, int t) {
    DiscLayout L;
    int m = 0;
    long long off = 0;
    auto put = [&](int C, int H, int p) {
        L.off[m] = off;
        L.C[m] = C; L.H[m] = H; L.p[m] = p;
        off += up16((long long)N * p * C * H);
        ++m;
    };
    int T = t;
    put(kSCh[0], T, 1);
    for (int i = 1; i < 5; ++i) { T = (T - 1) / 4 + 1; put(kSCh[i], T, 1); }
    put(kSCh[5], T, 1);
    put(1, T, 1);
    for (int d = 0; d < 5; ++d) {
        const int p = kPeriods[d];
        int H = cdiv(t, p);
        for (int i = 0; i < 4; ++i) { H = cdiv(H, 3); put(kPCh[i], H, p); }
        put(kPCh[4], H, p);
        put(1, H, p);
    }
    L.off[m] = off;
    return L;
}

long long flowvae_stage_work_floats(int B, int T, int seg, int hop) {
    const DiscLayout L = disc_layout(2 * B, seg * hop);
    return up16((long long)B * seg * hop) + up16((long long)B * 128 * T) + 2 * up16((long long)B * 128 * seg) + L.off[DISC_MAPS] + 64;
}

const float* Model::DW(const std::string& name, size_t numel) const {
    auto it = disc_weights_.find(name);
    if (it == disc_weights_.end()) throw Error(-4, "weight '" + name + "' missing from the bound discriminator blob");
    if (it->second.second != numel)
        throw Error(-4, "weight '" + name + "': expected " + std::to_string(numel) + " floats, the discriminator blob has " + std::to_string(it->second.second));
    return it->second.first;
}

PackedConv Model::disc_conv(const std::string& name, int Cin, int Cout, int KW) const {
    PackedConv pc;
    pc.Cin = Cin;
    pc.CinP = round_up(Cin, 16);
    pc.Cout = Cout;
    pc.CoutP = packed_cout(Cout);
    pc.KW = KW;
    pc.w = DW(name + ".wp", (size_t)KW * pc.CinP * pc.CoutP);
    pc.b = DW(name + ".bp", (size_t)pc.CoutP);
    return pc;
}

void Model::bind_discriminator(const void* blob, size_t nbytes, const char* const* names, const unsigned long long* offsets,
                               const unsigned long long* numels, int n, hipStream_t) {
    DTTS_REQUIRE(blob && names && offsets && numels && n > 0, "bind_discriminator: null argument");
    has_disc_ = false;
    disc_weights_.clear();
    for (int i = 0; i < n; ++i) {
        DTTS_REQUIRE((offsets[i] + numels[i]) * sizeof(float) <= nbytes, "weight table entry outside the discriminator blob");
        DTTS_REQUIRE(offsets[i] % 4 == 0, "weight offsets must be 16-byte aligned");
        disc_weights_[names[i]] = {static_cast<const float*>(blob) + offsets[i], (size_t)numels[i]};
    }
    DiscW d;
    const std::string s0 = "discriminators.0.";
    d.sw[0] = DW(s0 + "convs.0.weight", 16 * 15);
    d.sb[0] = DW(s0 + "convs.0.bias", 16);
    for (int i = 1; i < 5; ++i) {
        const int cin_g = kSCh[i - 1] / kSGroups[i];
        d.sw[i] = DW(s0 + "convs." + std::to_string(i) + ".weight", (size_t)kSCh[i] * cin_g * 41);
        d.sb[i] = DW(s0 + "convs." + std::to_string(i) + ".bias", (size_t)kSCh[i]);
    }
    d.s5 = disc_conv(s0 + "convs.5", 1024, 1024, 5);
    d.s_post = disc_conv(s0 + "conv_post", 1024, 1, 3);
    for (int k = 0; k < 5; ++k) {
        const std::string p = "discriminators." + std::to_string(k + 1) + ".";
        d.per[k].w0 = DW(p + "convs.0.weight", 32 * 5);
        d.per[k].b0 = DW(p + "convs.0.bias", 32);
        for (int i = 1; i < 4; ++i)       // stride 3: the 2-tap conv over the de-interleaved input (disc.h)
            d.per[k].c[i - 1] = disc_conv(p + "convs." + std::to_string(i), 3 * kPCh[i - 1], kPCh[i], 2);
        d.per[k].c[3] = disc_conv(p + "convs.4", 1024, 1024, 5);
        d.per[k].post = disc_conv(p + "conv_post", 1024, 1, 3);
    }
    disc_ = d;
    has_disc_ = true;
}

void Model::disc_forward(const float* y, const float* y_hat, int B, int t, float* maps, hipStream_t s) {
    DTTS_REQUIRE(has_disc_, kNoDisc);
    DTTS_REQUIRE(y && maps, "disc_forward: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 1024, "disc_forward: batch size");
    DTTS_REQUIRE(t >= 12 && t <= (1 << 24), "disc_forward: t must be at least 12 samples (every reflect pad shorter than the signal)");
    const int N = y_hat ? 2 * B : B;
    const DiscLayout L = disc_layout(N, t);
    // scratch: the split waveform (at most t + 10 samples per row) and the largest de-interleaved operand
    size_t dein = 0;
    for (int d = 0; d < 5; ++d)
        for (int i = 0; i < 3; ++i) {
            const int m = 7 + 6 * d + i;
            dein = std::max(dein, (size_t)N * L.p[m] * 3 * L.C[m] * cdiv(L.H[m], 3));
        }
    ArenaUse use_stage_c_arena(ws_voc_);
    ws().ensure(sizeof(float) * ((size_t)N * (t + 11) + dein) + 8192);
    float* xs = ws().f32((size_t)N * (t + 11));
    float* dx = ws().f32(dein);
    auto gemm = [&](const PackedConv& pc, const float* x, int cin, int Tin, float* out, int cout, int Nout, int R, int pad, bool act) {
        ConvParams p = cp(x, cin, Tin, Tin, nullptr, out, cout, Nout, Nout, nullptr, R);
        p.pad = pad;
        if (act) { p.epi_act = ACT_LRELU; p.epi_slope = DISC_SLOPE; }
        run_conv(pc, p, s);
    };
    // ---- DiscriminatorS on the N rows as they are
    launch_period_split(y, y_hat, B, N, t, 1, xs, s);
    launch_disc_first(xs, disc_.sw[0], disc_.sb[0], N, t, 16, 15, 1, 7, DISC_SLOPE, maps + L.off[0], L.H[0], s);
    for (int i = 1; i < 5; ++i)
        launch_conv1d_grouped(maps + L.off[i - 1], disc_.sw[i], disc_.sb[i], N, kSCh[i - 1], L.H[i - 1], kSCh[i], kSGroups[i], 41, 4, 20, DISC_SLOPE,
                              maps + L.off[i], L.H[i], s);
    gemm(disc_.s5, maps + L.off[4], 1024, L.H[4], maps + L.off[5], 1024, L.H[5], N, 2, true);
    gemm(disc_.s_post, maps + L.off[5], 1024, L.H[5], maps + L.off[6], 1, L.H[6], N, 1, false);
    // ---- DiscriminatorP: (K, 1) convs over [N, C, H, p] = plain conv1d over H on N p independent rows, kept as [N][p][C][H]
    for (int d = 0; d < 5; ++d) {
        const int p = kPeriods[d], R = N * p, m0 = 7 + 6 * d, H0 = cdiv(t, p);
        const DiscPeriodW& w = disc_.per[d];
        launch_period_split(y, y_hat, B, N, t, p, xs, s);
        launch_disc_first(xs, w.w0, w.b0, R, H0, 32, 5, 3, 2, DISC_SLOPE, maps + L.off[m0], L.H[m0], s);
        for (int i = 1; i < 4; ++i) {
            const int mi = m0 + i - 1, M = cdiv(L.H[mi], 3);         // M == L.H[mi + 1]
            launch_deinterleave3(maps + L.off[mi], R, L.C[mi], L.H[mi], dx, s);
            gemm(w.c[i - 1], dx, 3 * L.C[mi], M, maps + L.off[mi + 1], L.C[mi + 1], M, R, 1, true);
        }
        gemm(w.c[3], maps + L.off[m0 + 3], 1024, L.H[m0 + 3], maps + L.off[m0 + 4], 1024, L.H[m0 + 4], R, 2, true);
        gemm(w.post, maps + L.off[m0 + 4], 1024, L.H[m0 + 4], maps + L.off[m0 + 5], 1, L.H[m0 + 5], R, 1, false);
    }
}

void Model::disc_losses(int n_maps, const float* const* r, const float* const* g, const long long* map_numel, int n_scores,
                        const float* const* dr, const float* const* dg, const long long* score_numel, float* out, hipStream_t s) {
    DTTS_REQUIRE(has_disc_, kNoDisc);
    DTTS_REQUIRE(out && n_maps >= 0 && n_maps <= DISC_MAPS && n_scores >= 0 && n_scores <= DISC_COUNT && n_maps + n_scores >= 1,
                 "disc_losses: at most 37 maps and 6 scores, at least one of either");
    DTTS_REQUIRE(n_maps == 0 || (r && g && map_numel), "disc_losses: null map list");
    DTTS_REQUIRE(n_scores == 0 || (dg && score_numel), "disc_losses: null score list");
    LossItems items;
    for (int k = 0; k < n_maps; ++k) {
        DTTS_REQUIRE(r[k] && g[k] && map_numel[k] >= 1 && map_numel[k] < (1ll << 40), "disc_losses: an empty or null map");
        items.add(r[k], g[k], map_numel[k], LOSS_ABS_DIFF);
    }
    for (int pass = dr ? 0 : 1; pass < 3; ++pass)
        for (int k = 0; k < n_scores; ++k) {
            const float* a = pass == 0 ? dr[k] : dg[k];
            DTTS_REQUIRE(a && score_numel[k] >= 1 && score_numel[k] < (1ll << 40), "disc_losses: an empty or null score");
            items.add(a, nullptr, score_numel[k], pass == 1 ? LOSS_SQ : LOSS_ONE_MINUS_SQ);
        }
    DTTS_REQUIRE(items.blocks < (1 << 30), "disc_losses: sizes");
    ArenaUse use_stage_c_arena(ws_voc_);
    ws().ensure(sizeof(float) * ((size_t)items.blocks + LOSS_MAX_ITEMS) + 4096);
    float* partials = ws().f32((size_t)items.blocks);
    float* means = ws().f32(LOSS_MAX_ITEMS);
    launch_loss_means(items, partials, means, s);
    launch_disc_combine(means, n_maps, n_scores, dr ? 1 : 0, out, s);
}

void Model::spec_to_mel(const float* spec, int B, int spec_ch, int T, float* mel_out, hipStream_t s) {
    DTTS_REQUIRE(has_disc_, kNoDisc);      // the entries of this stage are one group: none of them runs before the discriminator is bound
    DTTS_REQUIRE(bound_ && has_frontend_, "front-end matrices not bound");
    DTTS_REQUIRE(spec && mel_out && B >= 1 && B <= 4096 && T >= 1 && T <= (1 << 20), "spec_to_mel: arguments");
    DTTS_REQUIRE(spec_ch == fe_nfft_ / 2 + 1, "spec_to_mel: the spectrogram's width is not that of the packed mel matrix (n_fft / 2 + 1)");
    ConvParams q = cp(spec, spec_ch, mel_out, cfg.mel_channels, B, T, T, nullptr);
    q.epi_act = ACT_LOG_CLAMP;
    run_conv(fe_mel_, q, s);
}

void Model::op_conv1d_grouped(const float* x, const float* w, const float* bias, int B, int Cin, int Tin, int Cout, int groups, int K, int stride,
                              int pad, float slope, float* y, hipStream_t s) {
    DTTS_REQUIRE(has_disc_, kNoDisc);
    DTTS_REQUIRE(x && w && y, "op_conv1d_grouped: null argument");
    DTTS_REQUIRE(Tin >= 1 && K >= 1 && stride >= 1 && pad >= 0 && Tin + 2 * pad >= K, "op_conv1d_grouped: the padded input is shorter than the kernel");
    launch_conv1d_grouped(x, w, bias, B, Cin, Tin, Cout, groups, K, stride, pad, slope, y, (Tin + 2 * pad - K) / stride + 1, s);
}

void Model::op_period_split(const float* wav, int B, int t, int p, float* out, hipStream_t s) {
    DTTS_REQUIRE(has_disc_, kNoDisc);
    DTTS_REQUIRE(wav && out, "op_period_split: null argument");
    DTTS_REQUIRE(B >= 1 && B <= 1024 && p >= 1 && p <= 64 && t > p && t <= (1 << 24), "op_period_split: the reflect pad (at most p - 1 samples) must be shorter than the signal");
    launch_period_split(wav, nullptr, B, B, t, p, out, s);
}

void Model::flowvae_stage_losses(const float* mel, const float* spec, int spec_ch, const int* lens_host, int B, int T, const float* noise,
                                 unsigned long long seed, const int* sample_ids_host, const int* ids_slice_host, int seg, const float* wav, int L,
                                 float* o, float* z, float* z_p, float* m_p, float* logs_p, float* m_q, float* logs_q, float* quantized,
                                 float* work, float* losses, hipStream_t s) {
    DTTS_REQUIRE(has_disc_, kNoDisc);
    DTTS_REQUIRE(bound_ && has_frontend_, "front-end matrices not bound");
    DTTS_REQUIRE(wav && work && losses && ids_slice_host, "flowvae_stage_losses: null argument");
    size_t hop = 1;
    for (int i = 0; i < cfg.n_upsamples; ++i) hop *= (size_t)cfg.upsample_rates[i];
    DTTS_REQUIRE(B >= 1 && T >= 1 && seg >= 1 && seg <= T && (long long)seg * hop <= (1 << 24), "flowvae_stage_losses: sizes");
    DTTS_REQUIRE((long long)L >= (long long)T * (long long)hop, "flowvae_stage_losses: wav must hold hop samples for every frame of mel");
    DTTS_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0, "flowvae_stage_losses: work must be 16-byte aligned");
    ArenaUse use_stage_c_arena(ws_voc_);
    // (flowvae_forward checks the rest, ids_slice included, before its first launch)
    flowvae_forward(mel, spec, spec_ch, lens_host, B, T, noise, seed, sample_ids_host, ids_slice_host, seg, o, z, z_p, m_p, logs_p, m_q, logs_q,
                    quantized, s);
    const int t = (int)(seg * hop), nm = cfg.mel_channels;
    float* ywav = work;
    float* mel_full = ywav + up16((long long)B * t);
    float* y_mel = mel_full + up16((long long)B * nm * T);
    float* yh_mel = y_mel + up16((long long)B * nm * seg);
    float* maps = yh_mel + up16((long long)B * nm * seg);
    const DiscLayout Lm = disc_layout(2 * B, t);
    float* scal = maps + Lm.off[DISC_MAPS];               // [0] mean |y_mel - y_hat_mel|, [16] the KL
    // y = slice_segments(wav, ids_slice * hop, segment_size)  (train.py:290)
    std::vector<int> wid(B);
    for (int b = 0; b < B; ++b) wid[b] = ids_slice_host[b] * (int)hop;
    slice_segments(wav, wid.data(), B, 1, L, t, ywav, s);
    // y_mel = slice_segments(spec_to_mel(spec), ids_slice, seg) ; y_hat_mel = mel_spectrogram(o)  (:268-288)
    spec_to_mel(spec, B, spec_ch, T, mel_full, s);
    slice_segments(mel_full, ids_slice_host, B, nm, T, seg, y_mel, s);
    mel_spectrogram(o, nullptr, B, t, fe_nfft_, (int)hop, yh_mel, seg, s);
    l1_mean(y_mel, yh_mel, B, nm, seg, scal, s);
    // D(y, y_hat) and the three losses  (:306-310)
    disc_forward(ywav, o, B, t, maps, s);
    const float *r[DISC_MAPS], *g[DISC_MAPS], *dr[DISC_COUNT], *dg[DISC_COUNT];
    long long mn[DISC_MAPS], sn[DISC_COUNT];
    int ns = 0;
    for (int m = 0; m < DISC_MAPS; ++m) {
        mn[m] = Lm.numel(m, B);
        r[m] = maps + Lm.off[m];
        g[m] = r[m] + mn[m];
        if (Lm.C[m] == 1) { dr[ns] = r[m]; dg[ns] = g[m]; sn[ns] = mn[m]; ++ns; }
    }
    disc_losses(DISC_MAPS, r, g, mn, ns, dr, dg, sn, losses, s);
    kl_loss(z_p, logs_q, m_p, logs_p, lens_host, B, cfg.inter_channels, T, scal + 16, s);
    launch_stage_combine(scal, scal + 16, losses, s);
}

}  // namespace dtts
