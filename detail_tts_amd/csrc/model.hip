// Model runtime core: workspace arenas, int upload ring, weight lookup and binding, the conv launch (see model.h).
#include "model.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace dtts {

// ------------------------------------------------------------------------------------------ Arena
static thread_local Arena* t_arena_override = nullptr;
Arena* arena_override() { return t_arena_override; }
ArenaUse::ArenaUse(Arena& a) : prev_(t_arena_override) { t_arena_override = &a; }
ArenaUse::~ArenaUse() { t_arena_override = prev_; }

static thread_local bool t_row_invariant = false;
RowInvariantLaunches::RowInvariantLaunches() : prev_(t_row_invariant) { t_row_invariant = true; }
RowInvariantLaunches::~RowInvariantLaunches() { t_row_invariant = prev_; }
bool RowInvariantLaunches::on() { return t_row_invariant; }

Arena::~Arena() {
    if (base_) (void)hipFree(base_);
}

void Arena::ensure(size_t bytes) {
    if (bytes > cap_) {
        DTTS_CHECK_HIP(hipDeviceSynchronize());
        if (base_) DTTS_CHECK_HIP(hipFree(base_));
        base_ = nullptr;
        cap_ = 0;
        const size_t want = bytes + bytes / 8 + (1u << 20);
        DTTS_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&base_), want));
        cap_ = want;
    }
    off_ = 0;
}

void* Arena::raw(size_t bytes) {
    const size_t a = (off_ + 255) & ~size_t(255);
    if (a + bytes > cap_) throw Error(-3, "workspace arena overflow (internal sizing bug)");
    off_ = a + bytes;
    return base_ + a;
}

// ------------------------------------------------------------------------------------------ Model
static constexpr size_t INT_RING_BYTES = 1u << 20;      // per issuing thread
Model::Model(const dtts_config& c, int dev) : cfg(c), device(dev) {
    DTTS_CHECK_HIP(hipSetDevice(dev));
    const long long mb = env_int("DTTS_UNCOND_CACHE_MB", 4096);
    ucache_want_ = (size_t)(mb < 0 ? 0 : mb) << 20;
}

Model::~Model() {
    gpt_drop_graphs();
    try { ucache_release(); } catch (...) {}
    if (x3_sat_) (void)hipHostFree(x3_sat_);
    for (auto& kv : int_rings_) {
        IntRing& r = *kv.second;
        if (r.dev) (void)hipFree(r.dev);
        if (r.pinned) (void)hipHostFree(r.pinned);
        if (r.ev) (void)hipEventDestroy(r.ev);
    }
    for (hipStream_t st : {sx_[0], sx_[1], sx_[2], sg_})
        if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : {ev_fork_, ev_joinx_[0], ev_joinx_[1], ev_joinx_[2], ev_g0_, ev_g1_})
        if (e) (void)hipEventDestroy(e);
}

namespace {
// live-column tables of the lengths arrays this host thread uploaded (Model::register_cols); an entry dies when upload_ints hands
// the address range of its lengths (or of the table itself) out again
struct ColTable {
    const int* lens = nullptr;      // device lengths [nb]
    const int* cols = nullptr;      // device table [prefix[nb]]
    int nb = 0, T = 0;
    std::vector<int> prefix;        // columns before sample b
};
thread_local std::vector<ColTable> t_col_tables;
static bool col_tables_on() {
    static const bool on = env_on("DTTS_CONV_COLS");
    return on;
}

// every ring a host thread owns (on any handle) is marked free when the thread exits
struct RingOwnerGuard {
    std::vector<std::shared_ptr<std::atomic<int>>> flags;
    ~RingOwnerGuard() {
        for (auto& f : flags) f->store(0);
    }
};
thread_local RingOwnerGuard t_ring_guard;
}  // namespace

Model::IntRing& Model::int_ring() {
    std::lock_guard<std::mutex> lk(ints_mu_);
    const auto me = std::this_thread::get_id();
    auto it = int_rings_.find(me);
    if (it == int_rings_.end() && int_rings_.size() >= MAX_INT_RINGS) {
        // hand on the least recently used ring of a thread that has EXITED (a live owner may be inside upload_ints holding a reference:
        // rings are not locked - ADVICE r04), after retiring every segment of it.  No such ring - a pool of more than 16 long-lived
        // workers that take turns on the handle, which the "two at a time" contract allows - means this thread gets a new
        // ring (2 MiB: 1 device + 1 pinned) beyond the soft cap; thread churn stays bounded because exited owners are recycled first.
        auto lru = int_rings_.end();
        for (auto j = int_rings_.begin(); j != int_rings_.end(); ++j)
            if (j->second->owner_alive->load() == 0 && (lru == int_rings_.end() || j->second->last_use < lru->second->last_use)) lru = j;
        if (lru != int_rings_.end()) {
            std::unique_ptr<IntRing> r = std::move(lru->second);
            int_rings_.erase(lru);
            for (auto& us : r->users) {
                for (hipStream_t u : us) {
                    if (hipEventRecord(r->ev, u) == hipSuccess) DTTS_CHECK_HIP(hipEventSynchronize(r->ev));
                    else (void)hipGetLastError();
                }
                us.clear();
            }
            r->off = 0;
            r->seg = 0;
            r->owner_alive.reset();
            int_rings_[me] = std::move(r);
        }
    }
    auto& slot = int_rings_[me];
    if (!slot) {
        slot.reset(new IntRing());
        DTTS_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&slot->dev), INT_RING_BYTES));
        DTTS_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&slot->pinned), INT_RING_BYTES, hipHostMallocDefault));
        DTTS_CHECK_HIP(hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming));
    }
    if (!slot->owner_alive || slot->owner_alive->load() == 0) {        // new ring, recycled ring, or a new thread that got an exited thread's id
        slot->owner_alive = std::make_shared<std::atomic<int>>(1);
        t_ring_guard.flags.push_back(slot->owner_alive);
    }
    slot->last_use = ++ring_clock_;
    return *slot;
}

const int* Model::upload_ints(const int* host, int n, hipStream_t s) {
    // Small host -> device int tables (lengths, ids, maps).  The copy goes through the thread's pinned mirror, so hipMemcpyAsync is
    // truly asynchronous (a pageable source makes the runtime stage - and wait - on the launch stream).  Lifetime: a table is read by
    // launches the calling thread enqueues on `s` after this call; its segment is handed out again only after an event recorded on
    // every stream that used it - at the time of reuse, i.e. behind those launches - has completed.
    constexpr size_t cap = INT_RING_BYTES / sizeof(int), seg_ints = cap / IntRing::SEGS;
    DTTS_REQUIRE(n >= 0 && (size_t)n <= cap / 4, "int table too large for the upload ring");
    IntRing& r = int_ring();
    const size_t len = (size_t)((n + 15) & ~15);
    if (r.off + len > cap) r.off = 0;
    const int first = (int)(r.off / seg_ints), last = (int)((r.off + (len ? len - 1 : 0)) / seg_ints);
    for (int g = first; g <= last; ++g) {
        if (g == r.seg && r.off != (size_t)g * seg_ints) continue;        // still inside the segment we are filling
        if (g != r.seg || r.off == (size_t)g * seg_ints) {               // entering segment g: retire its previous lap
            for (hipStream_t u : r.users[g]) {
                // a stream the caller has destroyed since is retired by definition (hipStreamDestroy completes its work): the
                // record fails with an invalid-handle error, which must not surface in an unrelated later call
                if (hipEventRecord(r.ev, u) == hipSuccess) DTTS_CHECK_HIP(hipEventSynchronize(r.ev));
                else (void)hipGetLastError();
            }
            r.users[g].clear();
            r.seg = g;
        }
    }
    for (int g = first; g <= last; ++g)
        if (std::find(r.users[g].begin(), r.users[g].end(), s) == r.users[g].end()) r.users[g].push_back(s);
    int* dst = r.dev + r.off;
    int* stage = r.pinned + r.off;
    r.off += len;
    for (size_t i = t_col_tables.size(); i-- > 0;) {                  // tables whose lengths (or own storage) lived here are stale now
        const ColTable& e = t_col_tables[i];
        auto hit = [&](const int* q, int m) { return q < dst + len && dst < q + m; };
        if (hit(e.lens, e.nb) || hit(e.cols, e.prefix.back())) t_col_tables.erase(t_col_tables.begin() + (long)i);
    }
    if (n > 0) {
        std::memcpy(stage, host, sizeof(int) * (size_t)n);
        DTTS_CHECK_HIP(hipMemcpyAsync(dst, stage, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    return dst;
}

void Model::register_cols(const int* lens_dev, const int* lens_host, int nb, int T, hipStream_t s) {
    for (size_t i = t_col_tables.size(); i-- > 0;)                      // a new table for these lengths replaces the old one; nb = 0 only forgets it
        if (t_col_tables[i].lens == lens_dev) t_col_tables.erase(t_col_tables.begin() + (long)i);
    if (!col_tables_on() || !opt_conv_cols_ || !lens_dev || !lens_host || nb <= 0 || cdiv(T, X3_BN) >= 256) return;
    const int nt = cdiv(T, X3_BN);
    ColTable e;
    e.prefix.assign(1, 0);
    std::vector<int> tab;
    for (int b = 0; b < nb; ++b) {
        const int live = std::min(nt, cdiv(std::max(lens_host[b], 0), X3_BN));
        for (int i = 0; i < live; ++i) tab.push_back(b << 8 | i);
        e.prefix.push_back((int)tab.size());
    }
    if ((int)tab.size() == nt * nb || tab.empty()) return;            // every column is live (or none: the launches exit at once anyway)
    e.cols = upload_ints(tab.data(), (int)tab.size(), s);            // (may retire older entries; never this one: not yet listed)
    e.lens = lens_dev;
    e.nb = nb;
    e.T = T;
    if (t_col_tables.size() >= 32) t_col_tables.erase(t_col_tables.begin());
    t_col_tables.push_back(std::move(e));
}

const float* Model::Wopt(const std::string& name, size_t numel) const {
    auto it = weights_.find(name);
    if (it == weights_.end()) return nullptr;
    if (it->second.second != numel)
        throw Error(-4, "weight '" + name + "': expected " + std::to_string(numel) + " floats, blob has " +
                            std::to_string(it->second.second));
    return it->second.first;
}

const float* Model::W(const std::string& name, size_t numel) const {
    const float* p = Wopt(name, numel);
    if (!p) throw Error(-4, "weight '" + name + "' missing from the bound blob");
    return p;
}

PackedConv Model::conv(const std::string& name, int Cin, int Cout, int KW, bool bias, int cout_p) const {
    PackedConv pc;
    pc.Cin = Cin;
    pc.CinP = round_up(Cin, 16);
    pc.Cout = Cout;
    pc.CoutP = cout_p ? cout_p : packed_cout(Cout);
    pc.KW = KW;
    pc.w = W(name + ".wp", (size_t)KW * pc.CinP * pc.CoutP);
    pc.b = bias ? W(name + ".bp", (size_t)pc.CoutP) : nullptr;
    return pc;
}

AttnBlockW Model::attn_block(const std::string& p, int C, int H) const {
    AttnBlockW a;
    a.C = C;
    a.H = H;
    a.gn_g = W(p + ".norm.weight", C);
    a.gn_b = W(p + ".norm.bias", C);
    a.qkv = conv(p + ".qkv", C, 3 * C, 1);
    a.proj = conv(p + ".proj_out", C, C, 1);
    a.bias_tab = W(p + ".bias_tab", (size_t)H * 129);
    return a;
}

ResBlockW Model::res_block(const std::string& p, int C, int index) const {
    ResBlockW r;
    r.index = index;
    r.gn1_g = W(p + ".in_layers.0.weight", C);
    r.gn1_b = W(p + ".in_layers.0.bias", C);
    r.c1 = conv(p + ".in_layers.2", C, C, 1);
    r.emb = conv(p + ".emb_layers.1", C, 2 * C, 1);
    r.gn2_g = W(p + ".out_layers.0.weight", C);
    r.gn2_b = W(p + ".out_layers.0.bias", C);
    r.c2 = conv(p + ".out_layers.3", C, C, 3);
    return r;
}

void Model::bind_weights(const void* blob, size_t nbytes, const char* const* names, const unsigned long long* offsets,
                         const unsigned long long* numels, int n, hipStream_t stream) {
    weights_.clear();
    bound_ = false;
    {   // a new generation of weights: nothing cached under the old one is served again (uncond_cache.h)
        std::lock_guard<std::mutex> lk(ucache_mu_);
        ++bind_gen_;
        ucache_.invalidate_all();
    }
    for (int i = 0; i < n; ++i) {
        DTTS_REQUIRE((offsets[i] + numels[i]) * sizeof(float) <= nbytes, "weight table entry outside the blob");
        DTTS_REQUIRE(offsets[i] % 4 == 0, "weight offsets must be 16-byte aligned");
        weights_[names[i]] = {static_cast<const float*>(blob) + offsets[i], (size_t)numels[i]};
    }
    if (weights_.count("diffusion.inp_block.wp")) build_diffusion(stream);
    has_vocoder_ = weights_.count("dec.conv_pre.wp") != 0;
    if (has_vocoder_) build_vocoder(stream);
    has_gpt_ = weights_.count("gpt.mel_head.wp") != 0;
    if (has_gpt_) build_gpt(stream);
    has_vq_ = weights_.count("quantizer.table") != 0;
    if (has_vq_) build_vq();
    has_frontend_ = weights_.count("frontend.dft.wp") != 0;
    if (has_frontend_) build_frontend();
    bound_ = true;
}

ConvParams Model::cp(const float* x, int cin, float* y, int cout, int B, int T, int Ta, const int* lens) const {
    return cp(x, cin, T, Ta, lens, y, cout, T, Ta, lens, B);
}

ConvParams Model::cp(const float* x, int cin, int Tin, int Tin_a, const int* len_in, float* y, int cout, int Nout, int Nout_a,
                     const int* len_out, int B) const {
    ConvParams p;
    p.B = B;
    p.Tin = Tin;
    p.Nout = Nout;
    p.len_in = len_in;
    p.len_out = len_out;
    p.x = x;
    p.x_bs = (long long)cin * Tin_a;
    p.x_cs = Tin_a;
    p.y = y;
    p.y_bs = (long long)cout * Nout_a;
    p.y_cs = Nout_a;
    return p;
}

// ragged batch: the live columns of the samples [b0, b0 + B) a split-precision trunk conv covers (register_cols)
static void attach_cols(ConvParams& p) {
    if (t_col_tables.empty() || !p.len_out || p.len_out != p.len_in || p.Nout != p.Tin || p.stride != 1 || p.phases != 1) return;
    for (const ColTable& e : t_col_tables)
        if (p.len_out >= e.lens && p.len_out + p.B <= e.lens + e.nb && p.Nout == e.T) {
            const int b0 = (int)(p.len_out - e.lens), c0 = e.prefix[b0], c1 = e.prefix[b0 + p.B];
            if (c1 > c0 && c1 - c0 < p.B * cdiv(p.Nout, X3_BN)) {
                p.cols = e.cols + c0;
                p.ncols = c1 - c0;
                p.cols_b0 = b0;
            }
            return;
        }
}

// (p.p1, the one-product mode of option "trunk_fp16", is the caller's: the trunk's blocks set it, everything else leaves it 0)
void Model::run_conv(const PackedConv& pc, ConvParams p, hipStream_t s, ConvX3Launch* chosen) const {
    p.w = pc.w;
    if (!p.bias) p.bias = pc.b;
    p.Cin = pc.Cin;
    p.CinP = pc.CinP;
    p.Cout = pc.Cout;
    p.CoutP = pc.CoutP;
    p.KW = pc.KW;
    if (p.x3) {
        DTTS_REQUIRE(pc.w3, "conv has no split-precision weights");
        p.w3 = pc.w3;
        attach_cols(p);
        if (RowInvariantLaunches::on()) p.ksplit_max = 1;
        launch_conv_x3(p, s, chosen);
        return;
    }
    launch_conv_gemm(p, s);
}

// Generic conv entry for parity tests.  In phases mode (ConvTranspose1d) Cout is the real channel count per phase,
// the packed weight holds phases*Cout rows and KW/pad describe the equivalent correlation (see packing.py).
void Model::op_conv1d(const char* name, const float* x, const int* lens_in_host, int B, int Cin, int Tin, int Cout, int KW,
                      int stride, int dil, int pad, int pro_act, int epi_act, int gate, int phases, const float* res, float* y,
                      int Tout_alloc, hipStream_t s) {
    DTTS_REQUIRE(!weights_.empty(), "weights not bound");
    const int rows = Cout * (phases > 1 ? phases : 1);
    PackedConv pc = conv(name, Cin, rows, KW, Wopt(std::string(name) + ".bp", (size_t)packed_cout(rows)) != nullptr);
    const int Nout = (Tin + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    std::vector<int> li(B), lo(B);
    for (int b = 0; b < B; ++b) {
        li[b] = lens_in_host ? lens_in_host[b] : Tin;
        lo[b] = (li[b] + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
    }
    const int* dli = upload_ints(li.data(), B, s);
    const int* dlo = upload_ints(lo.data(), B, s);
    const int cout_real = gate ? Cout / 2 : Cout;
    ConvParams p = cp(x, Cin, Tin, Tin, dli, y, cout_real, Nout, Tout_alloc, dlo, B);
    p.stride = stride;
    p.dil = dil;
    p.pad = pad;
    p.pro_act = pro_act;
    p.pro_slope = 0.1f;
    p.epi_act = epi_act;
    p.epi_slope = 0.1f;
    p.gate = gate;
    p.phases = phases > 1 ? phases : 1;
    if (res) with_res(p, res, p.y_bs, Tout_alloc);
    run_conv(pc, p, s);
}

// Single-conv entry of the split-precision kernel for parity tests: the weights are split into the workspace per call, the input
// planes are written with the lengths folded in (no affine, no activation) and a ragged batch goes through the live-column table as in
// the trunk.  Everything launch_conv_x3 and the split passes require is checked HERE, before the first launch or upload: a bad shape
// never reaches a kernel.
void Model::op_conv1d_x3(const char* name, const float* x, const int* lens_host, int B, int Cin, int T, int Cout, int KW, int epi_act,
                         float out_scale, int gate, const float* badd, const float* res, int p1, int ksplit_max, float* y,
                         ConvX3Launch* chosen, hipStream_t s) {
    DTTS_REQUIRE(!weights_.empty(), "weights not bound");
    DTTS_REQUIRE(name && x && y, "op_conv1d_x3: null argument");
    DTTS_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= (1 << 20) && Cin > 0 && Cin <= (1 << 16) && Cout > 0 && Cout <= (1 << 16), "op_conv1d_x3: sizes");
    DTTS_REQUIRE(KW == 1 || KW == 3, "op_conv1d_x3: k = 1 or k = 3 (same padding) only");
    DTTS_REQUIRE(Cin % 16 == 0, "op_conv1d_x3: input channels must be a multiple of 16 (one K-step; the split passes write 8-channel chunks)");
    const int CoutP = packed_cout(Cout);
    DTTS_REQUIRE(CoutP % 128 == 0, "op_conv1d_x3: packed output rows must be a multiple of the 128-row tile (Cout > 64)");
    DTTS_REQUIRE(p1 == 0 || p1 == 1, "op_conv1d_x3: p1 is 0 or 1");
    DTTS_REQUIRE(gate == GATE_NONE || gate == GATE_TANH_SIGMOID, "op_conv1d_x3: gate is none or tanh * sigmoid");
    DTTS_REQUIRE(!p1 || (Cin % 32 == 0 && gate == GATE_NONE), "op_conv1d_x3 one-product mode: input channels a multiple of 32, no gate");
    DTTS_REQUIRE(epi_act == ACT_NONE || epi_act == ACT_SILU || epi_act == ACT_LRELU || epi_act == ACT_TANH, "op_conv1d_x3: epilogue activation");
    DTTS_REQUIRE(ksplit_max >= 0, "op_conv1d_x3: ksplit_max");
    const bool rows16 = (reinterpret_cast<unsigned long long>(y) & 15ull) == 0 && T % 4 == 0;
    if (gate != GATE_NONE) {
        DTTS_REQUIRE(KW == 1 && !res && epi_act == ACT_NONE && out_scale == 1.f && Cout % 2 == 0,
                     "op_conv1d_x3 gated epilogue: 1x1 conv, no residual / activation / scale, an even number of rows");
        DTTS_REQUIRE(rows16, "op_conv1d_x3 gated epilogue: rows of y must be 16-byte aligned (T a multiple of 4)");
    } else {
        DTTS_REQUIRE(!badd, "op_conv1d_x3: badd only with the gate");
    }
    const int nt = cdiv(T, X3_BN);
    DTTS_REQUIRE((long long)(CoutP / 128) * nt * B <= (1 << 22), "op_conv1d_x3: launch too large");
    std::vector<int> l(B);
    for (int b = 0; b < B; ++b) {
        l[b] = lens_host ? lens_host[b] : T;
        DTTS_REQUIRE(l[b] >= 0 && l[b] <= T, "op_conv1d_x3: lengths must lie in [0, T]");
    }
    PackedConv pc = conv(name, Cin, Cout, KW, Wopt(std::string(name) + ".bp", (size_t)CoutP) != nullptr);
    DTTS_REQUIRE(pc.CinP == Cin && pc.CoutP == CoutP, "op_conv1d_x3: packed weight shape");
    // ---- nothing has been launched or uploaded up to here
    const size_t w3_bytes = (size_t)KW * (Cin / 8) * 2 * CoutP * 16;      // [tap][Cin/8][2 planes][CoutP] 16-byte chunks (conv_x3.h)
    ws().ensure(w3_bytes + x3_bytes(B, Cin, T) + 8192);
    void* w3 = ws().raw(w3_bytes);
    void* xs = ws().raw(x3_bytes(B, Cin, T));
    launch_split_weights(pc.w, KW, pc.CinP, pc.CoutP, w3, s);
    pc.w3 = w3;
    const int* dl = upload_ints(l.data(), B, s);
    const long long x_bs = (long long)Cin * T;
    launch_split_planes(x, x_bs, T, nullptr, ACT_NONE, dl, T, B, Cin, xs, s);
    register_cols(dl, l.data(), B, T, s);
    ConvParams p = cp(x, Cin, y, gate != GATE_NONE ? Cout / 2 : Cout, B, T, T, dl);
    p.pad = KW == 3 ? 1 : 0;
    p.epi_act = epi_act;
    p.epi_slope = 0.1f;
    p.out_scale = out_scale;
    p.gate = gate;
    if (badd) {
        p.badd = badd;              // [B][Cout] in packed row order
        p.badd_bs = Cout;
    }
    if (res) with_res(p, res, p.y_bs, T);
    with_planes(p, xs, T);
    p.p1 = p1;
    p.ksplit_max = ksplit_max;
    run_conv(pc, p, s, chosen);
    register_cols(dl, nullptr, 0, T, s);                               // enqueued: forget this call's table
}

// The trunk attention's split-precision path on its own, for parity tests: split_weights -> split_planes (no affine, no activation,
// lengths folded in) -> conv_x3 writing the Q / K / V operand images (EPI 2) -> flash_attn_x3b on those images, on one stream.  `name`
// is a packed 1 x 1 conv of 144 H rows in QKVAttentionLegacy order; bias_tab is a DEVICE [H][129] table in AttnParams::bias_tab's
// convention.  y receives the attention output before proj_out in the production form - the proj conv's input planes
// [B][6 H][2][x3_tp(T)][8 fp16] (zero-filled here first: the kernel's contract is that unwritten columns keep the previous writer's
// zeros) - or, out_f32, as fp32 rows [B][48 H][T].  That fp32 epilogue exists in flash_attn_x3b_kernel but the trunk never reaches it
// today (attention_block takes the planes form whenever T + 1 < x3_tp(T), which always holds); it is kept, and reachable from here
// only.  The image buffer is filled with 0xFF bytes (every fp16 a NaN) before the conv: in production it holds whatever its previous
// user left, so the conv and the attention must agree exactly on which chunks are live; img_out (may be null) receives a copy.
// Everything the launches require is checked before the first launch or upload.  No kernel and no production launch changes for this.
void Model::op_attention_x3(const char* name, const float* x, const int* lens_host, int B, int Cin, int T, int H, const float* bias_tab,
                            int p1, int out_f32, void* y, void* img_out, ConvX3Launch* conv_chosen, AttnX3Launch* attn_chosen, hipStream_t s) {
    DTTS_REQUIRE(!weights_.empty(), "weights not bound");
    DTTS_REQUIRE(name && x && y && bias_tab, "op_attention_x3: null argument");
    DTTS_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= (1 << 16) && Cin > 0 && Cin <= (1 << 16) && H > 0 && H <= 64, "op_attention_x3: sizes");
    DTTS_REQUIRE(Cin % 16 == 0, "op_attention_x3: input channels must be a multiple of 16 (one K-step; the split passes write 8-channel chunks)");
    DTTS_REQUIRE(p1 == 0 || p1 == 1, "op_attention_x3: p1 is 0 or 1");
    DTTS_REQUIRE(!p1 || Cin % 32 == 0, "op_attention_x3 one-product mode: input channels a multiple of 32");
    constexpr int D = AttnPlanes::D;
    const int Cout = 3 * D * H, CoutP = packed_cout(Cout);
    DTTS_REQUIRE(CoutP % 128 == 0, "op_attention_x3: packed rows");
    DTTS_REQUIRE((long long)(CoutP / 128) * cdiv(T, X3_BN) * B <= (1 << 22) && (long long)cdiv(T, 128) * H * B <= (1 << 22), "op_attention_x3: launch too large");
    DTTS_REQUIRE((reinterpret_cast<unsigned long long>(y) & 15ull) == 0 && (!img_out || (reinterpret_cast<unsigned long long>(img_out) & 15ull) == 0),
                 "op_attention_x3: 16-byte aligned outputs");
    std::vector<int> l(B);
    for (int b = 0; b < B; ++b) {
        l[b] = lens_host ? lens_host[b] : T;
        DTTS_REQUIRE(l[b] >= 0 && l[b] <= T, "op_attention_x3: lengths must lie in [0, T]");
    }
    const size_t w3_bytes = (size_t)(Cin / 8) * 2 * CoutP * 16, xs_bytes = x3_bytes(B, Cin, T), img_bytes = AttnPlanes::bytes(B, H, T);
    const size_t out_bytes = out_f32 ? (size_t)B * H * D * T * sizeof(float) : x3_bytes(B, H * D, T);
    DTTS_REQUIRE(w3_bytes + xs_bytes + img_bytes <= ((size_t)1 << 31), "op_attention_x3: workspace beyond 2 GiB");
    PackedConv pc = conv(name, Cin, Cout, 1, true);
    DTTS_REQUIRE(pc.CinP == Cin && pc.CoutP == CoutP && pc.w && pc.b, "op_attention_x3: packed weight shape (144 H rows, with bias)");
    // ---- nothing has been launched or uploaded up to here
    ws().ensure(w3_bytes + xs_bytes + img_bytes + 8192);
    void* w3 = ws().raw(w3_bytes);
    void* xs = ws().raw(xs_bytes);
    void* img = ws().raw(img_bytes);
    DTTS_CHECK_HIP(hipMemsetAsync(img, 0xFF, img_bytes, s));
    if (!out_f32) DTTS_CHECK_HIP(hipMemsetAsync(y, 0, out_bytes, s));
    launch_split_weights(pc.w, 1, pc.CinP, pc.CoutP, w3, s);
    pc.w3 = w3;
    const int* dl = upload_ints(l.data(), B, s);
    launch_split_planes(x, (long long)Cin * T, T, nullptr, ACT_NONE, dl, T, B, Cin, xs, s);
    register_cols(dl, l.data(), B, T, s);
    ConvParams p = cp(x, Cin, static_cast<float*>(img), Cout, B, T, T, dl);
    with_planes(p, xs, T);
    p.p1 = p1;
    p.qkv_planes = img;                                  // as attention_block sets them
    p.qkv_heads = H;
    p.qkv_nt64 = AttnPlanes::nt64(T);
    p.qkv_tq = AttnPlanes::tq(T);
    p.qkv_qscale = (1.f / std::sqrt((float)D)) * 1.4426950408889634f;
    run_conv(pc, p, s, conv_chosen);
    register_cols(dl, nullptr, 0, T, s);                 // enqueued: forget this call's table
    if (img_out) DTTS_CHECK_HIP(hipMemcpyAsync(img_out, img, img_bytes, hipMemcpyDeviceToDevice, s));
    AttnParams a;
    a.qkv = static_cast<const float*>(img);
    a.lens = dl;
    a.T = T;
    a.B = B;
    a.H = H;
    a.D = D;
    a.scale = 1.f / std::sqrt((float)D);
    a.bias_tab = bias_tab;
    a.planes = img;
    a.p1 = p1;
    if (out_f32) {
        a.out = static_cast<float*>(y);
        a.o_bs = (long long)H * D * T;
        a.o_cs = T;
    } else {
        a.out_x3 = y;
        a.x3_tp = x3_tp(T);
    }
    launch_flash_attention(a, s, attn_chosen);
}

// What both fp32 attention unit entries check before anything is launched or uploaded; fills l[b] (null lens -> T).
static void attn_f32_args(const char* who, const int* lens_host, int B, int rows, int cs, int T, int H, int D, int q_off, int k_off,
                          int v_off, int head_stride, std::vector<int>& l) {
    const std::string w(who);
    DTTS_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= (1 << 16) && H > 0 && H <= 64 && rows > 0 && rows <= (1 << 16), (w + ": sizes").c_str());
    DTTS_REQUIRE(D == 48 || D == 64 || D == 96 || D == 192, (w + ": head dim outside the launcher's set (48, 64, 96, 192)").c_str());
    DTTS_REQUIRE(cs >= T && cs <= (1 << 17), (w + ": the row stride must be at least T").c_str());
    DTTS_REQUIRE(head_stride >= 0 && head_stride <= rows, (w + ": head stride").c_str());
    const int offs[3] = {q_off, k_off, v_off};
    for (int off : offs)
        DTTS_REQUIRE(off >= 0 && (long long)off + (long long)(H - 1) * head_stride + D <= rows, (w + ": q / k / v rows leave the tensor").c_str());
    DTTS_REQUIRE((long long)cdiv(T, 128) * H * B <= (1 << 22), (w + ": launch too large").c_str());
    l.resize(B);
    for (int b = 0; b < B; ++b) {
        l[b] = lens_host ? lens_host[b] : T;
        DTTS_REQUIRE(l[b] >= 0 && l[b] <= T, (w + ": lengths must lie in [0, T]").c_str());
    }
}

// ONE launch_flash_attention on the caller's fp32 rows, for parity tests (tests/test_gpu_attn_f32.py): flash_attn_kernel<D, MODE> of
// csrc/attention.hip with D in {48, 64, 96, 192} and MODE plain / T5 bias table / causal / VITS rel-key band, exactly as the four
// production call sites drive it (GPT prefill, enc_p, MelStyleEncoder, the trunk under conv_x3 = 0).  qkv DEVICE [B][rows][cs], cs >= T
// (the trunk's Ta); row of (head h, dim c) = off + h * head_stride + c.  y DEVICE [B][H D][T] and ml DEVICE [B][H][T][2] (may be null)
// are the caller's, written at columns t < len only.  bias_tab DEVICE [H][129], band DEVICE [B][H][T][2 band_w + 1]; at most one of
// bias_tab, causal, band (the launcher has no kernel for a combination).  A sample of length 0 is legal: its workgroups return at once.
// Everything is checked before the first launch or upload.  No kernel and no production launch changes for this.
void Model::op_attention(const float* qkv, const int* lens_host, int B, int rows, int cs, int T, int H, int D, int q_off, int k_off,
                         int v_off, int head_stride, float scale, const float* bias_tab, int causal, const float* band, int band_w,
                         float* y, float* ml, hipStream_t s) {
    DTTS_REQUIRE(qkv && y, "op_attention: null argument");
    std::vector<int> l;
    attn_f32_args("op_attention", lens_host, B, rows, cs, T, H, D, q_off, k_off, v_off, head_stride, l);
    DTTS_REQUIRE(causal == 0 || causal == 1, "op_attention: causal is 0 or 1");
    DTTS_REQUIRE((bias_tab ? 1 : 0) + causal + (band ? 1 : 0) <= 1, "op_attention: at most one of bias table, causal and band");
    DTTS_REQUIRE(band ? (band_w >= 0 && 2 * band_w + 1 <= 16) : band_w == 0, "op_attention: band window (2 W + 1 <= 16; 0 without a band)");
    DTTS_REQUIRE(std::isfinite(scale), "op_attention: scale");
    // ---- nothing has been launched or uploaded up to here
    AttnParams a;
    a.qkv = qkv;
    a.bs = (long long)rows * cs;
    a.cs = cs;
    a.q_off = q_off;
    a.k_off = k_off;
    a.v_off = v_off;
    a.head_stride = head_stride;
    a.out = y;
    a.o_bs = (long long)H * D * T;
    a.o_cs = T;
    a.lens = upload_ints(l.data(), B, s);
    a.T = T;
    a.B = B;
    a.H = H;
    a.D = D;
    a.scale = scale;
    a.bias_tab = bias_tab;
    a.causal = causal;
    a.band = band;
    a.band_w = band_w;
    a.ml_out = ml;
    launch_flash_attention(a, s);
}

// The windowed relative-position attention of enc_p alone (vqvae/modules/attentions.py:161-303 MultiHeadAttention.attention, minus the
// convs): launch_vits_rel_key -> the band-mode flash kernel with ml_out -> launch_vits_rel_value, with the strides, offsets and buffers
// of Model::enc_p_fwd: qkv DEVICE [B][3 H D][T] as blocks [Q | K | V] of all heads (q_off 0, k_off H D, v_off 2 H D, head stride D,
// row stride T), ek / ev DEVICE [2 W + 1][D] (emb_rel_k / emb_rel_v, already sliced to the window), scale multiplies q . k and q . ek.
// y DEVICE [B][H D][T], relk DEVICE [B][H][T][2 W + 1] and ml DEVICE [B][H][T][2] are the caller's, written at t < len only.
void Model::op_attention_rel(const float* qkv, const int* lens_host, int B, int T, int H, int D, const float* ek, const float* ev, int W,
                             float scale, float* y, float* relk, float* ml, hipStream_t s) {
    DTTS_REQUIRE(qkv && ek && ev && y && relk && ml, "op_attention_rel: null argument");
    DTTS_REQUIRE(H > 0 && H <= 64 && (D == 48 || D == 64 || D == 96 || D == 192), "op_attention_rel: heads / head dim outside the launcher's set (48, 64, 96, 192)");
    const int hid = H * D;
    std::vector<int> l;
    attn_f32_args("op_attention_rel", lens_host, B, 3 * hid, T, T, H, D, 0, hid, 2 * hid, D, l);
    DTTS_REQUIRE(W >= 1 && 2 * W + 1 <= 16, "op_attention_rel: window (1 <= W, 2 W + 1 <= 16)");
    DTTS_REQUIRE(std::isfinite(scale), "op_attention_rel: scale");
    // ---- nothing has been launched or uploaded up to here
    const int* dl = upload_ints(l.data(), B, s);
    launch_vits_rel_key(qkv, (long long)3 * hid * T, T, 0, D, ek, relk, dl, B, H, D, T, W, scale, s);
    AttnParams at;
    at.qkv = qkv;
    at.bs = (long long)3 * hid * T;
    at.cs = T;
    at.q_off = 0;
    at.k_off = hid;
    at.v_off = 2 * hid;
    at.head_stride = D;
    at.out = y;
    at.o_bs = (long long)hid * T;
    at.o_cs = T;
    at.lens = dl;
    at.T = T;
    at.B = B;
    at.H = H;
    at.D = D;
    at.scale = scale;
    at.band = relk;
    at.band_w = W;
    at.ml_out = ml;
    launch_flash_attention(at, s);
    launch_vits_rel_value(qkv, (long long)3 * hid * T, T, 0, hid, D, relk, ml, ev, y, (long long)hid * T, T, dl, B, H, D, T, W, scale, s);
}

void Model::op_philox_normal(float* out, int n, int B, unsigned long long seed, const int* sample_ids_host, int stage, int step,
                             hipStream_t s) {
    const int* sids = upload_ints(sample_ids_host, B, s);
    launch_philox_normal(out, n, n, B, seed, sids, stage, step, 1.f, s);
}

}  // namespace dtts
