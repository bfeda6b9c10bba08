// Launch plan of the stacked-hourglass pose network (reference models/asn_stacked_hg.py:11-347):
// declaration of the parameter table in the reference's state_dict order, workspace layout, forward,
// hand-written backward and gradient reduction.  See net.h.
#include "net.h"
#include <stdio.h>

// PA_ABLATE=<mask> (tuning builds only; results are WRONG, timing bounds only: the most that fusing a launch kind into its neighbours can
// return).  The bits that leave a launch of each kind out: `always`; `k1` / `k3` by kernel size; `big1` / `big3` by kernel size on maps of
// >= 16384 pixels; `low` on maps up to PA_ABLATE_H (default 8) pixels high (what the low-resolution stretch costs the step at most)
enum { PA_L_SLAB_REDUCE, PA_L_CONV_WGRAD, PA_L_BN_FIN_FWD, PA_L_BN_FIN_BWD, PA_L_FWD_SITE, PA_L_CONV_FWD, PA_L_CONV_DGRAD, PA_L_UPADD_BWD,
       PA_L_POOL_BWD, PA_L_POOL_UPADD_FWD, PA_L_STEM_ROUTE };
static const struct { int always, k1, k3, big1, big3, low; } ablate_bits[] = {
    /* PA_L_SLAB_REDUCE     */ {1, 0, 0, 0, 0, 0},              // slab reductions of the weight-gradient stream
    /* PA_L_CONV_WGRAD      */ {2, 0, 0, 32, 64, 512},
    /* PA_L_BN_FIN_FWD      */ {4, 0, 0, 0, 0, 0},              // finalize launches
    /* PA_L_BN_FIN_BWD      */ {4, 0, 0, 0, 0, 256},
    /* PA_L_FWD_SITE        */ {0, 0, 0, 0, 0, 128},            // a forward convolution WITH its finalize, uncounted
    /* PA_L_CONV_FWD        */ {0, 0, 8, 0, 0, 0},
    /* PA_L_CONV_DGRAD      */ {0, 16, 8, 0, 0, 256},
    /* PA_L_UPADD_BWD       */ {1024, 0, 0, 0, 0, 0},           // (and no fused low-resolution half in the data gradient above it)
    /* PA_L_POOL_BWD        */ {2048, 0, 0, 0, 0, 0},           // (and no routing of the hourglass pools)
    /* PA_L_POOL_UPADD_FWD  */ {4096, 0, 0, 0, 0, 0},
    /* PA_L_STEM_ROUTE      */ {2048 | 16 | 4, 0, 0, 0, 0, 0},  // the stem pool's routed form needs its three launches
};
bool Net::ablated(int kind, int k, int H, long M) const {
    const int mask = pa_tuning().ablate;
    if (!mask) return false;
    const auto& b = ablate_bits[kind]; const bool big = M >= 16384;
    return (mask & (b.always | (k == 1 ? b.k1 | (big ? b.big1 : 0) : 0) | (k == 3 ? b.k3 | (big ? b.big3 : 0) : 0) | (H <= pa_tuning().ablate_h ? b.low : 0))) != 0;
}

template <class F> int Net::account(const PaWork& w, F launch, bool skip, bool count_skipped) {
    if (!skip || count_skipped) cnt(w);
    ProfEntry* pe = w.cls >= 0 ? prof.begin(w.cls, w.bytes, w.flops, st) : nullptr;
    const int rc = skip ? 0 : launch();
    prof.end(pe, st);
    return rc;
}

PaOperand pa_plain(const bf16* p) { PaOperand o; o.p = p; o.q = nullptr; o.k0 = o.k1 = o.k2 = nullptr; o.map = nullptr; o.mode = PA_LD_PLAIN; return o; }
PaOperand pa_none() { PaOperand o; o.p = o.q = nullptr; o.k0 = o.k1 = o.k2 = nullptr; o.map = nullptr; o.mode = PA_LD_NONE; return o; }
static int round64(int v) { return (v + 63) / 64 * 64; }
static PaWorkOp wop(const PaOperand& o) { return PaWorkOp{o.mode, o.q != nullptr}; }
static PaWorkConv wconv(const ConvLayer& c, int B, int H, int W) { return PaWorkConv{B, H, W, c.Cin, c.Cout, c.pcin, c.pcout, c.k, c.splits}; }

// ------------------------------------------------------------------------------------------------
// declaration
size_t Net::add_param(const std::string& name, std::initializer_list<int> shape) {
    TensorInfo t; t.name = name; t.ndim = (int)shape.size(); t.is_buffer = 0;
    size_t n = 1; int i = 0;
    for (int s : shape) { t.shape[i++] = s; n *= (size_t)s; }
    for (; i < 4; ++i) t.shape[i] = 1;
    n_params = (n_params + 3) & ~(size_t)3;           // 16-byte aligned tensors (float4 bias loads)
    t.offset = n_params; t.numel = n;
    n_params += n;
    tensors.push_back(t);
    return t.offset;
}

size_t Net::add_buffer(const std::string& name, int C) {
    TensorInfo t; t.name = name; t.ndim = 1; t.shape[0] = C; t.shape[1] = t.shape[2] = t.shape[3] = 1; t.is_buffer = 1;
    t.offset = n_buffers; t.numel = (size_t)C;
    n_buffers += (size_t)C;
    tensors.push_back(t);
    return t.offset;
}

void Net::declare_conv(ConvLayer& c, const std::string& name, int cin, int cout, int k, bool bn_after) {
    c.Cin = cin; c.Cout = cout; c.k = k; c.has_bn_after = bn_after;
    c.pcin = (k == 7) ? 256 : round64(cin);
    c.pcout = round64(cout);
    c.p_w = add_param(name + ".weight", {cout, cin, k, k});
    c.p_b = add_param(name + ".bias", {cout});
    convs.push_back(&c);
}

void Net::declare_bn(BNLayer& b, const std::string& name, int C) {
    b.C = C;
    b.p_gamma = add_param(name + ".weight", {C});
    b.p_beta = add_param(name + ".bias", {C});
    b.b_rmean = add_buffer(name + ".running_mean", C);
    b.b_rvar = add_buffer(name + ".running_var", C);
    TensorInfo t; t.name = name + ".num_batches_tracked"; t.ndim = 0; t.shape[0] = t.shape[1] = t.shape[2] = t.shape[3] = 1;
    t.is_buffer = 2; t.offset = 0; t.numel = 1;
    tensors.push_back(t);
    bns.push_back(&b);
}

void Residual::declare(Net& n, const std::string& p, int cin_, int cout_, bool adapter) {
    cin = cin_; cout = cout_; has_adapter = adapter;
    const int mid = cout / 2;
    n.declare_conv(c1, p + "conv1", cin, mid, 1, true);  n.declare_bn(b1, p + "bn1", mid);
    n.declare_conv(c2, p + "conv2", mid, mid, 3, true);  n.declare_bn(b2, p + "bn2", mid);
    n.declare_conv(c3, p + "conv3", mid, cout, 1, true); n.declare_bn(b3, p + "bn3", cout);
    if (adapter) n.declare_conv(ad, p + "adapter", cin, cout, 1, true);     // feeds bn3: bias gradient is zero
}

void Chain::declare(Net& n, const std::string& p, int chan, int modules) {
    m.resize(modules);                     // before the first block registers its layers: nothing moves afterwards
    for (int j = 0; j < modules; ++j) m[j].declare(n, p + std::to_string(j) + ".", chan, chan, false);
}

void Hourglass::declare(Net& n, const std::string& p, int chan) {
    // registration order of the reference (:56-68): "<site>.<j>." for the num_modules blocks of a site
    const char* dn[4] = {"down1.", "down2.", "down3.", "down4."};
    const char* un[4] = {"up1.", "up2.", "up3.", "up4."};
    const char* sn[4] = {"skip1.", "skip2.", "skip3.", "skip4."};
    for (int k = 0; k < 4; ++k) down[k].declare(n, p + dn[k], chan, n.modules);
    for (int k = 0; k < 4; ++k) up[k].declare(n, p + un[k], chan, n.modules);
    for (int k = 0; k < 4; ++k) skip[k].declare(n, p + sn[k], chan, n.modules);
    neck.declare(n, p + "neck.", chan, n.modules);
}

void Net::declare_pose() {
    declare_conv(stem_conv, "conv1", 3, 64, 7, true);
    declare_bn(stem_bn, "bn1", 64);
    res1.declare(*this, "residual1.", 64, 128, true);
    res2.declare(*this, "residual2.", 128, 128, false);
    res3.declare(*this, "residual3.", 128, chan, true);
    hg.resize(stacks); post.resize(stacks); lin.resize(stacks); lin_bn.resize(stacks); outc.resize(stacks);
    forth.resize(stacks > 0 ? stacks - 1 : 0); inc.resize(stacks > 0 ? stacks - 1 : 0);
    char buf[64];
    for (int i = 0; i < stacks; ++i) { snprintf(buf, sizeof buf, "hg.%d.", i); hg[i].declare(*this, buf, chan); }
    for (int i = 0; i < stacks; ++i) { snprintf(buf, sizeof buf, "post_res.%d.", i); post[i].declare(*this, buf, chan, modules); }
    for (int i = 0; i < stacks; ++i) {
        snprintf(buf, sizeof buf, "linear.%d.0", i); declare_conv(lin[i], buf, chan, chan, 1, true);
        snprintf(buf, sizeof buf, "linear.%d.1", i); declare_bn(lin_bn[i], buf, chan);
    }
    for (int i = 0; i < stacks; ++i) { snprintf(buf, sizeof buf, "out_conv.%d", i); declare_conv(outc[i], buf, chan, classes, 1, false); }
    for (int i = 0; i + 1 < stacks; ++i) { snprintf(buf, sizeof buf, "forth_conv.%d", i); declare_conv(forth[i], buf, chan, chan, 1, false); }
    for (int i = 0; i + 1 < stacks; ++i) { snprintf(buf, sizeof buf, "in_conv.%d", i); declare_conv(inc[i], buf, classes, chan, 1, false); }
    n_params = (n_params + 3) & ~(size_t)3;
}

// ------------------------------------------------------------------------------------------------
// workspace layout
void Net::layout_conv(ConvLayer& c, Arena& a, int M, int H, int W) {
    if (H <= 0 && B > 0) {                     // the net's own layers are square maps
        const int hw = M / B;
        int h = 1; while (h * h < hw) ++h;
        if (h * h == hw && hw * B == M) H = W = h;
    }
    const size_t wn = (size_t)c.pcout * (c.k == 7 ? 1 : c.taps()) * c.pcin;
    c.wf = a.get<bf16>(wn);
    c.wb = (c.k == 7) ? nullptr : a.get<bf16>(wn);
    // slab count (wgrad_plan.h): the grouped kernel's few, long splits where the layer's launches will be jobs of a group
    const bool shaped = H > 0 && W > 0 && M % (H * W) == 0;
    const PaWgradPlan p = pa_wgrad_plan(shaped ? M / (H * W) : M, shaped ? H : 0, shaped ? W : 0, c.pcin, c.pcout, c.k == 7 ? 1 : c.taps(), c.k == 7);
    c.splits = pa_wgrad_layer_splits(p, H > 0 && B > 0 && M == B * H * W);
    c.part_floats = (size_t)c.splits * wn;
    c.db_floats = c.has_bn_after ? 0 : (size_t)c.splits * c.pcout;
    c.part = a.get<float>(c.part_floats);
    c.dbpart = c.db_floats ? a.get<float>(c.db_floats) : nullptr;
}

void Net::layout_bn(BNLayer& b, Arena& a, int M) {
    b.max_rows = pa_max_stat_rows(M);
    b.stats = a.get<float>((size_t)b.max_rows * b.C * 2);
    b.bstats = a.get<float>((size_t)b.max_rows * b.C * 2);
    b.scale = a.get<float>(b.C); b.shift = a.get<float>(b.C); b.mean = a.get<float>(b.C); b.invstd = a.get<float>(b.C);
    b.kA = a.get<float>(b.C); b.kB = a.get<float>(b.C); b.kC = a.get<float>(b.C);
}

Act Net::new_act(Arena& a, int B_, int H, int W, int C, BNLayer* bn, bool need_grad) {
    Act t; t.B = B_; t.H = H; t.W = W; t.C = C; t.bn = bn;
    t.raw = a.get<bf16>(t.numel());
    t.grad = need_grad ? a.get<bf16>(t.numel()) : nullptr;
    return t;
}

void Residual::layout(Net& n, Arena& a, int B, int H, int W, bool need_grad) {
    const int M = B * H * W, mid = cout / 2;
    n.layout_conv(c1, a, M, H, W); n.layout_conv(c2, a, M, H, W); n.layout_conv(c3, a, M, H, W);      // explicit map size: the split counts depend on it
    n.layout_bn(b1, a, M); n.layout_bn(b2, a, M); n.layout_bn(b3, a, M * b3_rows_scale);
    x1 = n.new_act(a, B, H, W, mid, &b1, need_grad);
    x2 = n.new_act(a, B, H, W, mid, &b2, need_grad);
    x3 = n.new_act(a, B, H, W, cout, &b3, need_grad);
    dz3 = need_grad ? a.get<bf16>(x3.numel()) : nullptr;
    dz2 = need_grad ? a.get<bf16>(x2.numel()) : nullptr;
    if (has_adapter) {
        n.layout_conv(ad, a, M, H, W);
        adout = a.get<bf16>((size_t)M * cout);
        adgrad = need_grad ? a.get<bf16>((size_t)M * cin) : nullptr;
    }
}

void Chain::layout(Net& n, Arena& a, int B, int H, int W, bool need_grad, int tail_b3_rows_scale) {
    tail().b3_rows_scale = tail_b3_rows_scale;
    for (Residual& r : m) r.layout(n, a, B, H, W, need_grad);
}

void Hourglass::layout(Net& n, Arena& a, int B, int H, int W, bool need_grad) {
    const int C = n.chan;
    for (int k = 0; k < 4; ++k) {
        skip[k].layout(n, a, B, H >> k, W >> k, need_grad);
        pooled[k] = n.new_act(a, B, H >> (k + 1), W >> (k + 1), C, nullptr, need_grad);
        down[k].layout(n, a, B, H >> (k + 1), W >> (k + 1), need_grad);
        poolgrad[k] = need_grad ? a.get<bf16>((size_t)B * (H >> k) * (W >> k) * C) : nullptr;
        poolmap[k] = need_grad ? a.get<unsigned char>(pooled[k].numel()) : nullptr;
    }
    neck.layout(n, a, B, H >> 4, W >> 4, need_grad);
    for (int k = 3; k >= 0; --k) {
        // (the backward reductions of its last block can come from the data gradient over merged[k], 4 x the pixels: Residual::low_of_in)
        up[k].layout(n, a, B, H >> (k + 1), W >> (k + 1), need_grad, 4);
        merged[k] = n.new_act(a, B, H >> k, W >> k, C, nullptr, need_grad);
    }
    for (int k = 0; k < 4; ++k) skipm[k] = n.new_act(a, B, H >> k, W >> k, C, nullptr, need_grad);
    neckm = n.new_act(a, B, H >> 4, W >> 4, C, nullptr, need_grad);
}

size_t Net::layout_all(char* base) {
    Arena a; a.base = base;
    // region zeroed at the start of every step: BatchNorm statistic accumulators + per-stack loss
    size_t zero_begin = a.off;
    loss_dev = a.get<float>(64);
    a.take(0);
    stats_arena = base ? reinterpret_cast<float*>(base + zero_begin) : nullptr;
    stats_arena_floats = (a.off - zero_begin) / sizeof(float);
    loss_keep = a.get<float>(64);
    loss_self_clearing = true;                 // (the workspace is zero-filled when it is bound: the first pass starts from zero too)
    // job tables
    prep_jobs = a.get<PaPrepJob>(convs.size());
    red_jobs = a.get<PaWgradReduceJob>(convs.size());
    bneval_jobs = a.get<PaBnEvalJob>(bns.size());

    const int H2 = res / 2, H4 = res / 4;
    img4 = a.get<bf16>((size_t)B * res * res * 4);
    pts_dev = a.get<double>((size_t)B * classes * 2);
    layout_conv(stem_conv, a, B * H2 * H2);
    layout_bn(stem_bn, a, B * H2 * H2);
    a0 = new_act(a, B, H2, H2, 64, &stem_bn, true);
    res1.layout(*this, a, B, H2, H2, true);
    pool0 = new_act(a, B, H4, H4, 128, nullptr, true);
    stem_map = a.get<unsigned char>(pool0.numel());
    stem_xmax = a.get<bf16>(pool0.numel());
    res2.layout(*this, a, B, H4, H4, true);
    res3.layout(*this, a, B, H4, H4, true);
    lin_out.resize(stacks); xin.resize(stacks); heat.resize(stacks); heat_peak.resize(stacks); heat_peak_valid.assign(stacks, 0); heat64.resize(stacks); dheat64.resize(stacks);
    dheat_in.resize(stacks); forth_tmp.resize(stacks); lgrad_tmp.resize(stacks);
    const int M = B * H4 * H4;
    for (int i = 0; i < stacks; ++i) {
        hg[i].layout(*this, a, B, H4, H4, true);
        post[i].layout(*this, a, B, H4, H4, true);
        layout_conv(lin[i], a, M, H4, H4); layout_bn(lin_bn[i], a, M);
        lin_out[i] = new_act(a, B, H4, H4, chan, &lin_bn[i], true);
        layout_conv(outc[i], a, M, H4, H4);
        heat[i] = a.get<float>((size_t)M * 16);
        heat_peak[i] = a.get<float>((size_t)B * 16 * 2);
        heat64[i] = a.get<bf16>((size_t)M * 64);        // channels 16..63 stay zero (workspace is zero-filled once)
        dheat64[i] = a.get<bf16>((size_t)M * 64);
        dheat_in[i] = a.get<bf16>((size_t)M * 64);
        lgrad_tmp[i] = a.get<bf16>((size_t)M * chan);
        if (i + 1 < stacks) {
            layout_conv(forth[i], a, M, H4, H4); layout_conv(inc[i], a, M, H4, H4);
            forth_tmp[i] = a.get<bf16>((size_t)M * chan);
        }
        if (i == 0) xin[0] = res3.x3;
        if (i + 1 < stacks) xin[i + 1] = new_act(a, B, H4, H4, chan, nullptr, true);
    }
    a.take(0);
    return a.off;
}

int Net::upload_tables() {
    std::vector<PaPrepJob> pj; std::vector<PaWgradReduceJob> rj; std::vector<PaBnEvalJob> bj;
    prep_max = 0; red_max = 0;
    for (ConvLayer* c : convs) {
        PaPrepJob p; p.w = params + c->p_w; p.wf = c->wf; p.wb = c->wb; p.Cout = c->Cout; p.Cin = c->Cin;
        p.taps = c->k == 7 ? 49 : c->taps(); p.pad_cout = c->pcout; p.pad_cin = c->pcin;
        pj.push_back(p);
        int pe = c->pcout * (c->k == 7 ? 256 : c->taps() * c->pcin);
        if (pe > prep_max) prep_max = pe;
        if (c->k == 7) continue;
        PaWgradReduceJob r; r.part = c->part; r.dst = grads + c->p_w; r.dbpart = c->dbpart; r.dbdst = grads + c->p_b;
        r.Cout = c->pcout; r.Cin = c->pcin; r.taps = c->taps(); r.splits = c->splits; r.real_cout = c->Cout; r.real_cin = c->Cin;
        c->red_index = (int)rj.size();
        rj.push_back(r);
        int re = c->Cout * c->Cin * c->taps() + c->Cout;
        if (re > red_max) red_max = re;
    }
    for (BNLayer* b : bns) {
        PaBnEvalJob j; j.gamma = params + b->p_gamma; j.beta = params + b->p_beta; j.rmean = buffers + b->b_rmean;
        j.rvar = buffers + b->b_rvar; j.scale = b->scale; j.shift = b->shift; j.C = b->C;
        bj.push_back(j);
    }
    n_prep = (int)pj.size(); n_red = (int)rj.size(); n_bneval = (int)bj.size();
    PA_CHECK(hipMemcpyAsync(prep_jobs, pj.data(), pj.size() * sizeof(PaPrepJob), hipMemcpyHostToDevice, st));
    PA_CHECK(hipMemcpyAsync(red_jobs, rj.data(), rj.size() * sizeof(PaWgradReduceJob), hipMemcpyHostToDevice, st));
    PA_CHECK(hipMemcpyAsync(bneval_jobs, bj.data(), bj.size() * sizeof(PaBnEvalJob), hipMemcpyHostToDevice, st));
    PA_CHECK(hipStreamSynchronize(st));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// per-launch HIP-event timing (off unless bench.py asks for it)
ProfEntry* Prof::begin(int cls, double bytes, double flops, hipStream_t st) {
    if (!on) return nullptr;
    if (used == entries.size()) {
        ProfEntry e; e.cls = 0; e.bytes = e.flops = 0;
        if (hipEventCreate(&e.e0) != hipSuccess || hipEventCreate(&e.e1) != hipSuccess) return nullptr;
        entries.push_back(e);
    }
    ProfEntry* e = &entries[used++];
    e->cls = cls; e->bytes = bytes; e->flops = flops;
    hipEventRecord(e->e0, st);
    return e;
}

void Prof::end(ProfEntry* e, hipStream_t st) { if (e) hipEventRecord(e->e1, st); }

int Prof::report(double* out) {
    for (int i = 0; i < PA_PROF_NCLS * 4; ++i) out[i] = 0.0;
    last_seq.clear();
    for (size_t i = 0; i < used; ++i) last_seq.push_back(entries[i].cls);
    for (size_t i = 0; i < used; ++i) {
        ProfEntry& e = entries[i];
        hipError_t r = hipEventSynchronize(e.e1);
        if (r != hipSuccess) return (int)r;
        float ms = 0.f;
        r = hipEventElapsedTime(&ms, e.e0, e.e1);
        if (r != hipSuccess) return (int)r;
        out[e.cls * 4 + 0] += (double)ms; out[e.cls * 4 + 1] += 1.0; out[e.cls * 4 + 2] += e.bytes; out[e.cls * 4 + 3] += e.flops;
    }
    used = 0;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// runtime helpers
PaOperand Net::op(const Act& a) const {
    PaOperand o = pa_plain(a.raw);
    if (a.bn) { o.mode = PA_LD_BNRELU; o.k0 = a.bn->scale; o.k1 = a.bn->shift; }
    return o;
}

PaOperand Net::gradop(const Act& a) const {
    PaOperand o = pa_plain(a.grad);
    if (a.bn) { o.mode = PA_LD_LIN2; o.q = a.raw; o.k0 = a.bn->kA; o.k1 = a.bn->kB; o.k2 = a.bn->kC; }
    return o;
}

PaEpilogue Net::final_ep(const Act& a) const {
    PaEpilogue e = ep_plain();
    if (a.bn) {
        e.mode = PA_OUT_BWD; e.stats = a.bn->bstats; e.rows_out = &a.bn->bstat_rows; e.xref = a.raw; e.scale = a.bn->scale; e.shift = a.bn->shift;
        e.mean = a.bn->mean; e.invstd = a.bn->invstd;
    }
    return e;
}

int Net::finish_grad(const Act& a) {
    if (!a.bn || ablated(PA_L_BN_FIN_BWD, 0, a.H)) return 0;
    return pa_launch_bn_fin(fin_bwd(*a.bn, a.M()), a.bn->C, st);
}

// defer: the only next reader of a's BatchNorm-backward constants is a data-gradient launch that takes the pending finalize
int Net::finish_grad_or_defer(const Act& a, bool defer) {
    if (fin_can_wait(a.bn, defer, true)) { a.bn->bfin_pending = true; return 0; }
    return finish_grad(a);
}

int Net::finish_grad2_or_defer(const Act& a, bool defer_a, const Act& b, bool defer_b) {
    const bool da = fin_can_wait(a.bn, defer_a, true), db = fin_can_wait(b.bn, defer_b, true);
    if (da) a.bn->bfin_pending = true;
    if (db) b.bn->bfin_pending = true;
    if (da || db) return da && db ? 0 : finish_grad(da ? b : a);
    return finish_grad2(a, b);
}

// the first reader of x3's BatchNorm-backward constants is conv3's data gradient (Residual::bwd_a), launched on whatever stream runs the
// block's backward pass; its weight gradient and the shortcut addend come later
bool Net::x3_fin_ok(const Residual& r, const Act& in) const { return (fin_mask & 4) && !drop_mask && fin_consumer_ok(r.c3, in.B, in.H, in.W, true); }

int Net::finish_grad2(const Act& a, const Act& b) {
    if (ablated(PA_L_BN_FIN_BWD, 0, a.H)) return 0;
    if (!a.bn || !b.bn) { TRY(finish_grad(a)); return finish_grad(b); }
    return pa_launch_bn_fin2(fin_bwd(*a.bn, a.M()), a.bn->C, fin_bwd(*b.bn, b.M()), b.bn->C, st);
}

bool Net::fin_consumer_ok(const ConvLayer& c, int B_, int H, int W, bool dgrad) const {
    if (fin_rows_max <= 0 || !train_bn || c.k == 7) return false;
    if ((long)B_ * H * W > 64L * PA_FIN_SMALL_ROWS) return false;          // (no producer tiling leaves <= 128 rows above that)
    PaConvShape s{};
    s.B = B_; s.H = H; s.W = W; s.taps = c.taps(); s.cus = pa_conv_cus();
    s.Cin = dgrad ? c.pcout : c.pcin; s.Cout = dgrad ? c.pcin : c.pcout;
    s.in_mode = dgrad ? PA_LD_LIN2 : PA_LD_BNRELU;
    return pa_conv_plan(s).takes_fin;
}

PaBnFin Net::fin_fwd(const BNLayer& b, int M) const {
    PaBnFin f; memset(&f, 0, sizeof f);
    f.stats = b.stats; f.rows = b.stat_rows; f.bwd = 0; f.count = (float)M;
    f.gamma = params + b.p_gamma; f.beta = params + b.p_beta; f.rmean = buffers + b.b_rmean; f.rvar = buffers + b.b_rvar;
    f.scale = b.scale; f.shift = b.shift; f.mean = b.mean; f.invstd = b.invstd;
    f.momentum = momentum; f.eps = eps; f.update_running = bn_update;
    return f;
}

PaBnFin Net::fin_bwd(const BNLayer& b, int M) const {
    PaBnFin f; memset(&f, 0, sizeof f);
    f.stats = b.bstats; f.rows = b.bstat_rows; f.bwd = 1; f.count = (float)M;
    f.scale = b.scale; f.mean = b.mean; f.invstd = b.invstd;
    f.kA = b.kA; f.kB = b.kB; f.kC = b.kC; f.dgamma = grads + b.p_gamma; f.dbeta = grads + b.p_beta;
    return f;
}

int Net::conv_fwd(ConvLayer& c, const PaOperand& in, int B_, int H, int W, const PaOperand& add1, const PaOperand& add2,
                  bf16* out, BNLayer* bn_after, BNLayer* pending_in, bool defer_after) {
    PaConvArgs a; memset(&a, 0, sizeof a);
    if (pending_in && pending_in->fin_pending) { a.fin = fin_fwd(*pending_in, B_ * H * W); pending_in->fin_pending = false; }
    a.in = in; a.w = c.wf; a.bias = params + c.p_b; a.add1 = add1; a.add2 = add2; a.out = out; a.low_prio = on_side ? 1 : 0;
    a.B = B_; a.H = H; a.W = W; a.Cin = c.pcin; a.Cout = c.pcout; a.taps = c.k == 7 ? 1 : c.taps();
    a.ep = ep_plain();
    if (bn_after && train_bn) { a.ep.mode = PA_OUT_STATS; a.ep.stats = bn_after->stats; a.ep.rows_out = &bn_after->stat_rows; }
    if (ablated(PA_L_FWD_SITE, c.k, H)) return 0;
    const PaWork w = pa_work_conv_fwd(wconv(c, B_, H, W), wop(in), wop(add1), wop(add2));
    TRY(account(w, [&] { return c.k == 7 ? pa_launch_stem_conv(a, st) : pa_launch_conv(a, st); }, ablated(PA_L_CONV_FWD, c.k)));
    if (!bn_after || !train_bn) return 0;
    if (fin_can_wait(bn_after, defer_after, false)) { bn_after->fin_pending = true; return 0; }
    return ablated(PA_L_BN_FIN_FWD) ? 0 : pa_launch_bn_fin(fin_fwd(*bn_after, B_ * H * W), bn_after->C, st);
}

int Net::conv_dgrad(ConvLayer& c, const PaOperand& dy, int B_, int H, int W, const PaOperand& add1, const PaOperand& add2,
                    const PaEpilogue& ep, bf16* out, bf16* dz_out, bool* dz_done, BNLayer* pending_in, const Act* low, bool* low_done,
                    const PaEpilogue* pool_in_ep) {
    PaConvArgs a; memset(&a, 0, sizeof a);
    if (low_done) *low_done = false;
    if (pending_in && pending_in->bfin_pending) { a.fin = fin_bwd(*pending_in, B_ * H * W); pending_in->bfin_pending = false; }
    a.in = dy; a.w = c.wb; a.bias = nullptr; a.add1 = add1; a.add2 = add2; a.out = out; a.ep = ep; a.low_prio = on_side ? 1 : 0;
    a.B = B_; a.H = H; a.W = W; a.Cin = c.pcout; a.Cout = c.pcin; a.taps = c.taps();
    if (dy.mode == PA_LD_POOL) {                   // (Net::stem_route_ok read the plan: the instance stores dz)
        if (!pool_in_ep || !dz_out) { pa_set_error_msg("conv_dgrad: a pool-routed gradient needs its mask and a dz buffer"); return 1; }
        a.ep2 = *pool_in_ep;
    }
    if (dy.mode == PA_LD_POOL || dy.mode == PA_LD_LIN2) a.dz_out = dz_out;      // stored where the plan's instance does (PaConvPlan::stores_dz)
    // the low-resolution half of the upsample-add backward in this launch's epilogue (round 6): an instance of the row-tile 1x1 kernel
    if (low && dy.mode != PA_LD_POOL && pa_tuning().upadd_fuse && low->bn && !drop_mask && !ablated(PA_L_UPADD_BWD)) { a.out2 = low->grad; a.ep2 = final_ep(*low); }
    PaConvPlan p = pa_conv_plan(pa_conv_shape(a));
    if (a.out2 && p.path != PA_CVP_ROW_UP) { a.out2 = nullptr; memset(&a.ep2, 0, sizeof a.ep2); p = pa_conv_plan(pa_conv_shape(a)); }      // not that instance's launch: on its own
    const bool up = p.path == PA_CVP_ROW_UP; if (dz_done) *dz_done = p.stores_dz;
    const PaWork w = pa_work_conv_dgrad(wconv(c, B_, H, W), wop(dy), wop(add1), wop(add2), ep.mode, p.stores_dz, up);
    const bool skip = ablated(PA_L_CONV_DGRAD, c.k, H);      // (a skipped launch is not counted, and leaves the row count a producer would have)
    if (skip && a.ep.rows_out) *a.ep.rows_out = 1;
    if (!skip && up && low_done) *low_done = true;
    return account(w, [&] { return pa_launch_conv(a, p, st); }, skip, false);
}

int Net::conv_wgrad(ConvLayer& c, const PaOperand& dy, const PaOperand& x, int B_, int H, int W) {
    PaWgradArgs a; memset(&a, 0, sizeof a);
    a.dy = dy; a.x = x; a.part = c.part; a.dbpart = c.dbpart;
    a.B = B_; a.H = H; a.W = W; a.Cin = c.pcin; a.Cout = c.pcout; a.taps = c.k == 7 ? 1 : c.taps(); a.splits = c.splits;
    if (ablated(PA_L_CONV_WGRAD, c.k, H, (long)B_ * H * W)) return 0;
    const PaWork w = pa_work_conv_wgrad(wconv(c, B_, H, W), wop(dy), wop(x));
    // With a weight-gradient stream every launch is collected and leaves in flush_wgrads() on that stream -- except the stem's, the last
    // launch of the step: on the main stream, idle by then, it runs beside the weight-gradient queue's last reduction instead of behind it.
    // Without one (single-stream mode: bench.py's roofline leg, debugging) the launches the grouped kernel takes are collected too and
    // leave as the same group launches on the caller's stream -- per-class event times and the bitwise comparison of the stream modes
    // then see the kernels of the real step; the others are launched here and summed by reduce_grads().
    const bool aside = wgrads_aside();
    const bool stem_now = c.k == 7 && aside && pa_tuning().stem_on_main;
    const int job_wgs = c.k == 7 ? 0 : pa_wgrad_job_workgroups(a);
    if (aside ? !stem_now : job_wgs > 0) {
        PendingWgrad p; p.a = a; p.w = w; p.stem = c.k == 7; p.job_wgs = job_wgs; p.c = &c;
        pending_wgrads.push_back(p);
        cnt(w);      // (counted here; its profile entry opens where it is launched: launch_pending_wgrads)
        return 0;
    }
    TRY(account(w, [&] { return c.k == 7 ? pa_launch_stem_wgrad(a, st) : pa_launch_wgrad(a, st); }));
    if (stem_now) TRY(pa_launch_stem_wgrad_reduce(c.part, c.splits, grads + c.p_w, st, grads + c.p_b));
    return 0;
}

int Net::flush_red_stash(hipStream_t ws) {
    red_stash_flushes = 0;
    if (red_stash.empty()) return 0;
    const int rc = pa_launch_wgrad_reduce_list(red_jobs, red_stash.data(), (int)red_stash.size(), red_stash_mx, ws);
    red_stash.clear(); red_stash_mx = 0;
    return rc;
}

void Net::drop_wgrads() {
    pending_wgrads.clear();
    red_stash.clear(); red_stash_mx = 0; red_stash_flushes = 0;
}

// Operands of the collected launches are final on `st` at this point (their producers were enqueued before).  The
// gradient buffers they read are written once per step, so deferring a launch is always safe.
int Net::flush_wgrads() {
    if (pending_wgrads.empty()) return 0;
    const int rc = launch_pending_wgrads();
    if (rc) drop_wgrads(); else pending_wgrads.clear();
    return rc;
}

int Net::launch_pending_wgrads() {
    const PaTuning& t = pa_tuning();
    const bool aside = wgrads_aside();
    hipStream_t ws = aside ? wstream : st;
    if (aside) {
        hipEvent_t ev = ev_w[ev_w_next]; ev_w_next = (ev_w_next + 1) & 15;
        PA_CHECK(hipEventRecord(ev, st));
        PA_CHECK(hipStreamWaitEvent(ws, ev, 0));
    }
    // slabs are summed on the weight-gradient stream as the step goes: the layers of a flush join the stash, and the stash is summed by a
    // few more workgroups of a LATER group launch of this stream (in_group) or by a launch of its own
    const bool stash = aside && !ablated(PA_L_SLAB_REDUCE), in_group = t.wg_red_in_group != 0;
    bool first = true;
    // every launch of the list the grouped kernel takes goes into group launches of up to 8 jobs (also while the per-launch event timing
    // runs: a group launch counts for the class of its largest job); the others -- the stem, shapes of the generic kernel -- are launched
    // one by one behind them
    std::vector<char> grouped(pending_wgrads.size(), 0);
    const PaWgradArgs* jobs[8]; int jidx[8]; int nj = 0;
    auto fire = [&]() -> int {
        if (nj == 0) return 0;
        // (event timing: the launch counts for the class of its largest job, with the bytes / flops of all of them)
        int big = 0; double bytes = 0.0, flops = 0.0;
        for (int j = 0; j < nj; ++j) {
            const PendingWgrad& q = pending_wgrads[jidx[j]];
            bytes += q.w.bytes; flops += q.w.flops;
            if (q.w.flops > pending_wgrads[jidx[big]].w.flops) big = j;
        }
        ProfEntry* pe = prof.begin(pending_wgrads[jidx[big]].w.cls, bytes, flops, ws);
        const bool carry = stash && in_group && !red_stash.empty();      // the slabs of EARLIER flushes ride in this launch
        const int rc = (nj == 1 && !carry) ? pa_launch_wgrad(*jobs[0], ws)
                                           : pa_launch_wgrad_group(jobs, nj, ws, false, red_jobs, carry ? red_stash.data() : nullptr, carry ? (int)red_stash.size() : 0);
        if (carry && !rc) { red_stash.clear(); red_stash_mx = 0; red_stash_flushes = 0; }
        prof.end(pe, ws);
        nj = 0; first = false;
        return rc;
    };
    // a group launch is capped at `cap` workgroups: its workgroups live for tens of microseconds with 242 registers each, two of them
    // close a CU to every other queue -- a launch of <= 256 leaves room for a workgroup of the main chain beside it on every CU
    const int cap = t.wg_group_cap;
    int wgs = 0;
    for (size_t pi = 0; pi < pending_wgrads.size(); ++pi) {
        PendingWgrad& p = pending_wgrads[pi];
        const int w = p.job_wgs;
        if (w == 0) continue;
        if (nj > 0 && (nj == 8 || wgs + w > cap)) { TRY(fire()); wgs = 0; }
        grouped[pi] = 1;
        jidx[nj] = (int)pi;
        jobs[nj++] = &p.a;
        wgs += w;
    }
    TRY(fire());
    // the ungrouped launches share no data: from the second on they need no completion / cache round trip behind their predecessor
    // (hipExtAnyOrderLaunch, conv_wgrad_tile.hip; not with the per-launch event timing, and not inside a stream capture -- the engine's
    // own or a caller's around pa_hg_backward: an extension launch cannot be captured)
    bool in_capture = capturing;
    if (!in_capture) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ws, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) in_capture = true;
    }
    for (size_t pi = 0; pi < pending_wgrads.size(); ++pi) {
        PendingWgrad& p = pending_wgrads[pi];
        if (grouped[pi]) continue;
        ProfEntry* pe = prof.begin(p.w.cls, p.w.bytes, p.w.flops, ws);
        pa_wgrad_set_launch_flags((t.wgrad_anyorder && !first && !prof.on && !in_capture) ? 1u : 0u);
        int rc = p.stem ? pa_launch_stem_wgrad(p.a, ws) : pa_launch_wgrad(p.a, ws);
        pa_wgrad_set_launch_flags(0u);
        first = false;
        prof.end(pe, ws);
        if (rc) return rc;
    }
    if (!stash) return 0;            // (no weight-gradient stream: reduce_grads() sums every slab at the end of the step)
    // the stash is summed every `lag`-th flush (one launch for the layers of two or three blocks: 41 reduction launches per step were
    // 0.3 - 0.6 ms of the weight-gradient queue), part of it still in the Infinity Cache; with in-group reductions it waits for the next
    // group launch, and gets a launch of its own only when none came for `lag` + 2 flushes
    const int lag = t.wreduce_lag < 1 ? 1 : t.wreduce_lag;
    for (PendingWgrad& p : pending_wgrads) {
        if (p.stem) { TRY(pa_launch_stem_wgrad_reduce(p.c->part, p.c->splits, grads + p.c->p_w, ws, grads + p.c->p_b)); continue; }
        const int el = p.c->Cout * p.c->Cin * p.c->taps() + p.c->Cout;
        if ((int)red_stash.size() == PA_RED_LIST_MAX) TRY(flush_red_stash(ws));
        red_stash.push_back(p.c->red_index);
        red_stash_mx = el > red_stash_mx ? el : red_stash_mx;
    }
    if (++red_stash_flushes >= (in_group ? lag + 2 : lag)) TRY(flush_red_stash(ws));
    return 0;
}

// the streaming launches with their operand bytes counted (Net::account, work_model.h); a skipped one leaves the row count its consumer waits for
static double elems(int B, int H, int W, int C) { return (double)B * H * W * C; }
static int c_maxpool_fwd(Net& n, const PaOperand& in, bf16* out, int B, int H, int W, int C, hipStream_t st, unsigned char* map = nullptr, bf16* xmax = nullptr) {
    return n.account(pa_work_maxpool_fwd(wop(in), elems(B, H, W, C), map != nullptr, xmax != nullptr),
                     [&] { return pa_launch_maxpool_fwd(in, out, B, H, W, C, st, map, xmax); }, n.ablated(PA_L_POOL_UPADD_FWD));
}
static int c_maxpool_bwd(Net& n, const bf16* dout, const PaOperand& in, const PaOperand& add, const PaEpilogue& ep, bf16* din, int B, int H, int W, int C,
                         hipStream_t st) {
    const bool skip = n.ablated(PA_L_POOL_BWD);
    if (skip && ep.rows_out) *ep.rows_out = 1;
    return n.account(pa_work_maxpool_bwd(wop(in), wop(add), ep.mode, elems(B, H, W, C)),
                     [&] { return pa_launch_maxpool_bwd(dout, in, add, ep, din, B, H, W, C, st); }, skip);
}
static int c_upadd_bwd(Net& n, const bf16* dout, const PaEpilogue& ep_low, bf16* dlow, const PaEpilogue& ep_skip, bf16* dskip, int B, int H, int W, int C,
                       hipStream_t st, int part = 3) {
    const bool skip = n.ablated(PA_L_UPADD_BWD);
    if (skip) { if (ep_low.rows_out && (part & 1)) *ep_low.rows_out = 1; if (ep_skip.rows_out && (part & 2)) *ep_skip.rows_out = 1; }
    return n.account(pa_work_upadd_bwd(elems(B, H, W, C), part, ep_low.mode, ep_skip.mode),
                     [&] { return pa_launch_upadd_bwd(dout, ep_low, dlow, ep_skip, dskip, B, H, W, C, st, nullptr, part); }, skip);
}

// ------------------------------------------------------------------------------------------------
// a scope whose launches go to stream `s` (a side branch)
struct StreamScope {
    Net& n; hipStream_t saved; bool saved_side;
    StreamScope(Net& n_, hipStream_t s) : n(n_), saved(n_.st), saved_side(n_.on_side) { n.st = s; n.on_side = true; }
    ~StreamScope() { n.st = saved; n.on_side = saved_side; }
};

// residual block (reference :30-49): x1 = conv1(a), x2 = conv3x3(relu bn1 x1), x3 = conv3(relu bn2 x2) + shortcut
int Residual::fwd(Net& n, const Act& in) {
    const int B = in.B, H = in.H, W = in.W;
    // x1 / x2 have ONE reader each (conv2 / conv3): at the low-resolution levels their BatchNorm finalize runs in that reader's prologue
    const bool d1 = (n.fin_mask & 1) && n.fin_consumer_ok(c2, B, H, W, false), d2 = (n.fin_mask & 1) && n.fin_consumer_ok(c3, B, H, W, false);
    TRY(n.conv_fwd(c1, n.op(in), B, H, W, pa_none(), pa_none(), x1.raw, &b1, nullptr, d1));
    TRY(n.conv_fwd(c2, n.op(x1), B, H, W, pa_none(), pa_none(), x2.raw, &b2, &b1, d2));
    if (has_adapter) {
        TRY(n.conv_fwd(ad, n.op(in), B, H, W, pa_none(), pa_none(), adout, nullptr));
        TRY(n.conv_fwd(c3, n.op(x2), B, H, W, pa_plain(adout), pa_none(), x3.raw, &b3, &b2));
    } else {
        TRY(n.conv_fwd(c3, n.op(x2), B, H, W, n.op(in), pa_none(), x3.raw, &b3, &b2));
    }
    return 0;
}

// precondition: x3.grad holds the finished masked gradient and finish_grad(x3) has run.
// bwd = bwd_a (parameter gradients and the inner data gradients) + bwd_b (gradient of the block input, the only
// part that needs `extra`, the gradient arriving at the input from its other consumers)
int Residual::bwd_a(Net& n, const Act& in) {
    const int B = in.B, H = in.H, W = in.W;
    low_fused = false;
    // conv3's data gradient goes first: its kernel also stores dz3 = BatchNorm-backward(x3.grad, x3.raw), and the weight
    // gradients / the shortcut addend after it read that one tensor instead of recomputing it from two
    // (x3.bn: its finalize may be pending -- then this launch does it in its prologue, Net::x3_fin_ok)
    PaOperand g3 = g3_pool_on ? g3_pool : n.gradop(x3);
    dz3_valid = false;
    TRY(n.conv_dgrad(c3, g3, B, H, W, pa_none(), pa_none(), n.final_ep(x2), x2.grad, dz3, &dz3_valid, x3.bn, nullptr, nullptr, g3_pool_on ? &g3_pool_ep : nullptr));
    if (g3_pool_on && !dz3_valid) { pa_set_error_msg("Residual::bwd_a: the pool-routed data gradient did not store dz3"); return 1; }
    if (dz3_valid) g3 = pa_plain(dz3);
    TRY(n.conv_wgrad(c3, g3, n.op(x2), B, H, W));
    // (x2's BatchNorm-backward constants are first read by conv2's data gradient, which can compute them in its prologue; conv2's
    // weight gradient, on the weight-gradient stream, is launched behind it)
    TRY(n.finish_grad_or_defer(x2, (n.fin_mask & 2) && n.fin_consumer_ok(c2, B, H, W, true)));
    PaOperand g2 = n.gradop(x2);
    dz2_valid = false;
    TRY(n.conv_dgrad(c2, g2, B, H, W, pa_none(), pa_none(), n.final_ep(x1), x1.grad, dz2, &dz2_valid, x2.bn));
    if (dz2_valid) g2 = pa_plain(dz2);
    TRY(n.conv_wgrad(c2, g2, n.op(x1), B, H, W));
    // (x1's constants have two first readers -- conv1's weight gradient on the weight-gradient stream and conv1's data gradient in bwd_b:
    // queueing the weight gradient behind a data gradient that finalizes in its prologue measured +0.05 ms, round 4 -- a launch stays)
    TRY(n.finish_grad(x1));
    const PaOperand g1 = n.gradop(x1);
    TRY(n.conv_wgrad(c1, g1, n.op(in), B, H, W));
    if (has_adapter) TRY(n.conv_wgrad(ad, g3, n.op(in), B, H, W));
    return n.flush_wgrads();                   // one event for the block's 3-4 weight gradients
}

int Residual::bwd_b(Net& n, const Act& in, const PaOperand& extra) {
    const int B = in.B, H = in.H, W = in.W;
    const PaOperand g3 = dz3_valid ? pa_plain(dz3) : n.gradop(x3), g1 = n.gradop(x1);
    if (has_adapter) {
        TRY(n.conv_dgrad(ad, g3, B, H, W, extra, pa_none(), ep_plain(), adgrad));
        TRY(n.conv_dgrad(c1, g1, B, H, W, pa_plain(adgrad), pa_none(), n.final_ep(in), in.grad));
    } else {
        TRY(n.conv_dgrad(c1, g1, B, H, W, g3, extra, n.final_ep(in), in.grad, nullptr, nullptr, nullptr, low_of_in, &low_fused));
    }
    return 0;
}

int Residual::bwd(Net& n, const Act& in, const PaOperand& extra, bool in_needs_grad) {
    TRY(bwd_a(n, in));
    return in_needs_grad ? bwd_b(n, in, extra) : 0;
}

// ------------------------------------------------------------------------------------------------
// chain of residual blocks: the launches the stem chains (residual2 -> residual3) and the hourglass chains (down4 -> neck)
int Chain::fwd(Net& n, const Act& in) {
    const Act* cur = &in;
    for (Residual& r : m) { TRY(r.fwd(n, *cur)); cur = &r.x3; }
    return 0;
}

// from the last block to the first; every block flushes its own weight gradients (Residual::bwd_a)
int Chain::bwd_a(Net& n, const Act& in) {
    for (int j = (int)m.size() - 1; j >= 1; --j) {
        const Act& bin = m[j - 1].x3;
        TRY(m[j].bwd(n, bin, pa_none(), true));
        TRY(n.finish_grad_or_defer(bin, n.x3_fin_ok(m[j - 1], j >= 2 ? m[j - 2].x3 : in)));
    }
    return m[0].bwd_a(n, in);
}

int Chain::bwd(Net& n, const Act& in, const PaOperand& extra, bool in_needs_grad) {
    TRY(bwd_a(n, in));
    return in_needs_grad ? bwd_b(n, in, extra) : 0;
}

// ------------------------------------------------------------------------------------------------
// hourglass (reference :139-157 down path, :192-203 up path)
// The skip branch of level k (a full-resolution residual block) does not depend on the low-resolution path
// below it: it is enqueued on the side stream and joined where its result is consumed.

int Hourglass::encode(Net& n, const Act& in) {
    const Act* cur = &in;
    for (int k = 0; k < 4; ++k) {
        auto skip_branch = [&]() -> int {
            TRY(skip[k].fwd(n, *cur));
            if (n.drop_mask) TRY(pa_launch_cell_mask(n.op(skip[k].out()), n.drop_mask, ep_plain(), skipm[k].raw, cur->B, cur->H, cur->W, cur->C, n.st));
            return 0;
        };
        if (n.multi_stream) {
            TRY(n.fork_to(k));
            { StreamScope sc(n, n.side); TRY(skip_branch()); }
            TRY(n.record_join(k));
        } else {
            TRY(skip_branch());
        }
        map_written[k] = n.maps_on && poolmap[k] != nullptr;
        TRY(c_maxpool_fwd(n, n.op(*cur), pooled[k].raw, cur->B, cur->H, cur->W, cur->C, n.st, map_written[k] ? poolmap[k] : nullptr));
        TRY(down[k].fwd(n, pooled[k]));
        cur = &down[k].out();
    }
    TRY(neck.fwd(n, *cur));
    if (n.drop_mask) {
        const Act& x = neck.out();
        TRY(pa_launch_cell_mask(n.op(x), n.drop_mask, ep_plain(), neckm.raw, x.B, x.H, x.W, x.C, n.st));
    }
    return 0;
}

int Hourglass::decode(Net& n) {
    const Act* low = n.drop_mask ? &neckm : &neck.out();
    for (int k = 3; k >= 0; --k) {
        TRY(up[k].fwd(n, *low));
        const Act& m = merged[k];
        if (n.multi_stream) TRY(n.wait_join(k));
        const PaOperand lo = n.op(up[k].out()), sk = n.op(n.drop_mask ? skipm[k] : skip[k].out());
        TRY(n.account(pa_work_upadd_fwd(wop(lo), wop(sk), (double)m.numel()), [&] { return pa_launch_upadd_fwd(lo, sk, m.raw, m.B, m.H, m.W, m.C, n.st); },
                      n.ablated(PA_L_POOL_UPADD_FWD)));
        low = &merged[k];
    }
    return 0;
}

bool Hourglass::low_fusable(const Net& n, int k) const {
    if (n.drop_mask || k < 0 || k > 3) return false;
    const Act& m = merged[k];
    return pa_upadd_bwd_splits(n.final_ep(up[k].out()), n.final_ep(skip[k].out()), m.B, m.H, m.W, m.C);
}

// Can the first block of skip[k] take the gradient of pool k through the arg-max map (its conv1 data gradient as Residual::bwd_b launches it:
// BatchNorm backward on load, dz3 or its LIN2 form as first addend, the epilogue of the block input x)?
bool Hourglass::route_ok(Net& n, int k, const Act& x, const PaOperand& ex0) {
    if (!(n.pool_route & 1) || !map_written[k] || n.ablated(PA_L_POOL_BWD)) return false;
    if (ex0.mode != PA_LD_NONE && ex0.mode != PA_LD_PLAIN) return false;
    Residual& r = skip[k].head();
    if (r.has_adapter || r.low_of_in) return false;
    PaConvShape s{};
    s.B = x.B; s.H = x.H; s.W = x.W; s.Cin = r.c1.pcout; s.Cout = r.c1.pcin; s.taps = r.c1.taps(); s.cus = pa_conv_cus();
    s.in_mode = n.gradop(r.x1).mode; s.add1_mode = PA_LD_PLAIN; s.add2_mode = PA_LD_POOL; s.add2_map = true; s.ep_mode = n.final_ep(x).mode;
    return pa_conv_plan(s).pool_route;
}

int Hourglass::fill_poolgrad(Net& n, int k, const Act& in) {
    const Act& x = (k == 0) ? in : down[k - 1].out();
    return pa_launch_maxpool_bwd(pooled[k].grad, n.op(x), route_extra[k], ep_plain(), poolgrad[k], x.B, x.H, x.W, x.C, n.st);
}

// precondition: merged[0].grad holds the finished (plain) gradient of the hourglass output.
// extra0: gradient reaching the hourglass INPUT from consumers outside the hourglass.
// Chains (num_modules > 1): merged[k] is read by the FIRST block of up[k-1] (its conv1 data gradient may emit d up[k].out() too: low_of_in /
// low_fused sit on head()), the upsample-add and the pool write the gradient of the LAST block of up[k] / skip[k] / down[k] (out()).  Of a skip
// chain only the first block's input gradient needs poolgrad[k]: everything else of the chain stays on the side stream (Chain::bwd_a).
int Hourglass::bwd(Net& n, const Act& in, const PaOperand& extra0) {
    for (int k = 0; k < 4; ++k) {
        const Act& m = merged[k];
        const Act& upo = up[k].out();
        const Act& sko = skip[k].out();
        // the two outputs of the upsample-add backward as two launches: d low on the main chain (the low-resolution path waits for it), d skip
        // on the side stream in front of the skip block's backward pass, its only reader -- the main chain waits for 75 MB instead of 175
        if (pa_tuning().upadd_split && !n.drop_mask && n.multi_stream && pa_upadd_bwd_splits(n.final_ep(upo), n.final_ep(sko), m.B, m.H, m.W, m.C)) {
            const Act& upin_ = (k == 3) ? neck.out() : merged[k + 1];
            const Act& x = (k == 0) ? in : down[k - 1].out();
            TRY(n.fork_to(k));
            {
                StreamScope sc(n, n.side);
                TRY(c_upadd_bwd(n, m.grad, n.final_ep(upo), upo.grad, n.final_ep(sko), sko.grad, m.B, m.H, m.W, m.C, n.st, 2));
                TRY(n.finish_grad_or_defer(sko, n.x3_fin_ok(skip[k], x)));
                TRY(skip[k].bwd_a(n, x));
            }
            TRY(n.record_join(k));
            // (d up[k].out() may have come out of the data gradient that produced d merged[k]: low_done)
            if (!low_done[k]) TRY(c_upadd_bwd(n, m.grad, n.final_ep(upo), upo.grad, n.final_ep(sko), sko.grad, m.B, m.H, m.W, m.C, n.st, 1));
            TRY(n.finish_grad_or_defer(upo, n.x3_fin_ok(up[k], upin_)));
            up[k].head().low_of_in = low_fusable(n, k + 1) ? &up[k + 1].out() : nullptr;
            TRY(up[k].bwd(n, upin_, pa_none(), true));
            if (k < 3) low_done[k + 1] = up[k].head().low_fused;
            continue;
        }
        if (n.drop_mask) {              // the skip tensor entered the sum through the cell mask: d skip = mask * d (masked skip)
            TRY(c_upadd_bwd(n, m.grad, n.final_ep(upo), upo.grad, ep_plain(), skipm[k].grad, m.B, m.H, m.W, m.C, n.st));
            TRY(pa_launch_cell_mask(pa_plain(skipm[k].grad), n.drop_mask, n.final_ep(sko), sko.grad, m.B, m.H, m.W, m.C, n.st));
        } else {
            // (low_done: only d skip is left -- the launch that can do one half exists wherever the fused data gradient does)
            TRY(c_upadd_bwd(n, m.grad, n.final_ep(upo), upo.grad, n.final_ep(sko), sko.grad,
                                    m.B, m.H, m.W, m.C, n.st, low_done[k] ? 2 : 3));
        }
        {
            const Act& upin_ = (k == 3) ? (n.drop_mask ? neckm : neck.out()) : merged[k + 1];
            const Act& skin_ = (k == 0) ? in : down[k - 1].out();
            TRY(n.finish_grad2_or_defer(upo, n.x3_fin_ok(up[k], upin_), sko, n.x3_fin_ok(skip[k], skin_)));
        }
        if (n.multi_stream) {          // parameter / inner gradients of the skip chain next to the deeper levels
            const Act& x = (k == 0) ? in : down[k - 1].out();
            TRY(n.fork_to(k));
            { StreamScope sc(n, n.side); TRY(skip[k].bwd_a(n, x)); }
            TRY(n.record_join(k));
        }
        const Act& upin = (k == 3) ? (n.drop_mask ? neckm : neck.out()) : merged[k + 1];
        up[k].head().low_of_in = low_fusable(n, k + 1) ? &up[k + 1].out() : nullptr;
        TRY(up[k].bwd(n, upin, pa_none(), true));
        if (k < 3) low_done[k + 1] = up[k].head().low_fused;
    }
    if (n.drop_mask) {
        const Act& x = neck.out();
        TRY(pa_launch_cell_mask(pa_plain(neckm.grad), n.drop_mask, n.final_ep(x), x.grad, x.B, x.H, x.W, x.C, n.st));
    }
    TRY(n.finish_grad_or_defer(neck.out(), n.x3_fin_ok(neck, down[3].out())));
    TRY(neck.bwd(n, down[3].out(), pa_none(), true));
    TRY(n.finish_grad_or_defer(down[3].out(), n.x3_fin_ok(down[3], pooled[3])));
    for (int k = 3; k >= 0; --k) {
        TRY(down[k].bwd(n, pooled[k], pa_none(), true));
        const Act& x = (k == 0) ? in : down[k - 1].out();
        // the pool's gradient reaches skip[k]'s first block through the arg-max map of the forward pool (no launch, no full-resolution tensor),
        // or as poolgrad[k] from a launch of its own
        const PaOperand ex0 = (k == 0) ? extra0 : pa_none();
        PaOperand pg = pa_plain(poolgrad[k]);
        routed[k] = route_ok(n, k, x, ex0);
        if (routed[k]) {
            route_extra[k] = ex0;
            pg.mode = PA_LD_POOL; pg.p = pooled[k].grad; pg.map = poolmap[k]; pg.q = ex0.mode == PA_LD_PLAIN ? ex0.p : nullptr;
        } else {
            TRY(c_maxpool_bwd(n, pooled[k].grad, n.op(x), ex0, ep_plain(), poolgrad[k], x.B, x.H, x.W, x.C, n.st));
        }
        if (n.multi_stream) {
            TRY(n.wait_join(k));
            TRY(skip[k].bwd_b(n, x, pg));
        } else {
            TRY(skip[k].bwd(n, x, pg, true));
        }
        if (k >= 1) TRY(n.finish_grad_or_defer(x, n.x3_fin_ok(down[k - 1], pooled[k - 1])));      // x = down[k-1].out(): read next by down[k-1]'s backward pass
        else TRY(n.finish_grad(x));
    }
    return 0;
}

int Net::ensure_streams() {
    if (streams_ready) return 0;
    if (pa_tuning().single_stream) { streams_ready = true; return 0; }      // (multi_stream is false from the start then)
    PA_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    for (int k = 0; k < 4; ++k) {
        PA_CHECK(hipEventCreateWithFlags(&ev_fork[k], hipEventDisableTiming));
        PA_CHECK(hipEventCreateWithFlags(&ev_join[k], hipEventDisableTiming));
    }
    if (!pa_tuning().no_wstream) {
        PA_CHECK(hipStreamCreateWithFlags(&wstream, hipStreamNonBlocking));
        for (int i = 0; i < 16; ++i) PA_CHECK(hipEventCreateWithFlags(&ev_w[i], hipEventDisableTiming));
        PA_CHECK(hipEventCreateWithFlags(&ev_wdone, hipEventDisableTiming));
    }
    streams_ready = true;
    return 0;
}
void Net::release_streams() {
    release_graph();
    if (bucket_events) { for (int i = 0; i < 16; ++i) (void)hipEventDestroy(ev_bucket[i]); (void)hipEventDestroy(ev_bucket_main); bucket_events = false; }
    if (mstream) { (void)hipStreamSynchronize(mstream); (void)hipStreamDestroy(mstream); (void)hipEventDestroy(ev_mfork); (void)hipEventDestroy(ev_meter); mstream = nullptr; meter_pending = false; }
    if (side) {
        (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); side = nullptr;
        for (int k = 0; k < 4; ++k) { (void)hipEventDestroy(ev_fork[k]); (void)hipEventDestroy(ev_join[k]); }
    }
    if (wstream) {
        (void)hipStreamSynchronize(wstream); (void)hipStreamDestroy(wstream); wstream = nullptr;
        for (int i = 0; i < 16; ++i) (void)hipEventDestroy(ev_w[i]);
        (void)hipEventDestroy(ev_wdone);
    }
    for (ProfEntry& e : prof.entries) { (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); }
    prof.entries.clear(); prof.used = 0;
    streams_ready = false;
}
int Net::fork_to(int k) { PA_CHECK(hipEventRecord(ev_fork[k], st)); PA_CHECK(hipStreamWaitEvent(side, ev_fork[k], 0)); return 0; }
int Net::record_join(int k) { PA_CHECK(hipEventRecord(ev_join[k], side)); return 0; }
int Net::wait_join(int k) { PA_CHECK(hipStreamWaitEvent(st, ev_join[k], 0)); return 0; }

// ------------------------------------------------------------------------------------------------
int Net::prepare_weights() { return pa_launch_weight_prep(prep_jobs, n_prep, prep_max, st); }

int Net::begin_step() {
    dbytes_rd = dbytes_wr = 0;
    if (!loss_self_clearing) PA_CHECK(hipMemsetAsync(stats_arena, 0, stats_arena_floats * sizeof(float), st));
    return 0;
}

// reference :282-342 (stem :283-289, stacks :292-334) + loss of stack-hg.py:156-159
int Net::meter_stream(hipStream_t* out) {
    *out = st;
    // a meter on the main stream may read what a pending meter-stream launch produced (the cached arg-max): order it behind them
    if (!meters_async || !multi_stream) return join_meters();
    if (!mstream) {
        PA_CHECK(hipStreamCreateWithFlags(&mstream, hipStreamNonBlocking));
        PA_CHECK(hipEventCreateWithFlags(&ev_mfork, hipEventDisableTiming));
        PA_CHECK(hipEventCreateWithFlags(&ev_meter, hipEventDisableTiming));
    }
    PA_CHECK(hipEventRecord(ev_mfork, st));
    PA_CHECK(hipStreamWaitEvent(mstream, ev_mfork, 0));
    *out = mstream;
    return 0;
}
int Net::meter_done(hipStream_t ms) {
    if (ms == st) return 0;
    PA_CHECK(hipEventRecord(ev_meter, ms));
    meter_pending = true;
    return 0;
}
int Net::join_meters() {
    if (!meter_pending) return 0;
    PA_CHECK(hipStreamWaitEvent(st, ev_meter, 0));
    meter_pending = false;
    return 0;
}

int Net::heat_argmax(int stack, const float** out, hipStream_t on) {
    const int H = res / 4;
    if (!heat_peak_valid[stack]) {
        TRY(pa_launch_argmax(heat[stack], (long)H * H * 16, 1, 16, B, 16, H, H, heat_peak[stack], nullptr, on ? on : st));
        heat_peak_valid[stack] = 1;
    }
    *out = heat_peak[stack];
    return 0;
}

int Net::forward_pose(const float* img_nchw, const bf16* img4_in, const double* pts, bool train, float* loss_out_dev) {
    const int rc = forward_pose_body(img_nchw, img4_in, pts, train, loss_out_dev);
    // the per-stack loss accumulators are cleared by the kernel that reads them at the END of a forward pass (loss_out_kernel): a pass that
    // fails after a head launch has added to them would leave its residue in every later loss -- clear them here then (self-healing)
    if (rc && pts && loss_dev && st) { (void)hipGetLastError(); (void)hipMemsetAsync(loss_dev, 0, 64 * sizeof(float), st); }
    return rc;
}

int Net::forward_pose_body(const float* img_nchw, const bf16* img4_in, const double* pts, bool train, float* loss_out_dev) {
    train_bn = train;
    heat_peak_valid.assign(stacks, 0);
    TRY(ensure_streams());
    TRY(join_meters());                 // (meters of the previous forward pass still read the heat maps this one overwrites)
    TRY(begin_step());
    if (!train) TRY(pa_launch_bn_eval(bneval_jobs, n_bneval, eps, st));
    const bf16* image = img4_in ? img4_in : img4;
    cur_image = image;
    if (!img4_in) TRY(pa_launch_nchw_to_nhwc4(img_nchw, img4, B, res, res, st));
    if (pts && pts != pts_dev) PA_CHECK(hipMemcpyAsync(pts_dev, pts, (size_t)B * classes * 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
    TRY(conv_fwd(stem_conv, pa_plain(image), B, res / 2, res / 2, pa_none(), pa_none(), a0.raw, &stem_bn));
    TRY(res1.fwd(*this, a0));
    // (with pool routing a training pass also stores the pools' arg-max maps, and the stem's pool the raw value at the arg-max)
    maps_on = (pool_route & 1) && train;
    stem_map_written = (pool_route & 2) && train && stem_map && pa_pool_stats_route_supported(op(res1.x3), final_ep(res1.x3), B, res / 2, res / 2, 128);
    TRY(c_maxpool_fwd(*this, op(res1.x3), pool0.raw, B, res / 2, res / 2, 128, st, stem_map_written ? stem_map : nullptr, stem_map_written ? stem_xmax : nullptr));
    TRY(res2.fwd(*this, pool0));
    TRY(res3.fwd(*this, res2.x3));
    const int Hh = res / 4;
    for (int i = 0; i < stacks; ++i) {
        TRY(hg[i].encode(*this, xin[i]));
        TRY(hg[i].decode(*this));
        TRY(post[i].fwd(*this, hg[i].out()));
        TRY(conv_fwd(lin[i], op(post[i].out()), B, Hh, Hh, pa_none(), pa_none(), lin_out[i].raw, &lin_bn[i]));
        TRY(account(pa_work_head_fwd(wop(op(lin_out[i])), elems(B, Hh, Hh, 1), chan), [&] {
            return pa_launch_head_fwd(op(lin_out[i]), outc[i].wf, params + outc[i].p_b, heat[i], heat64[i], pts ? pts_dev : nullptr, pts ? loss_dev + i : nullptr, B, Hh, Hh, chan, st); }));
        if (i + 1 < stacks) {
            TRY(conv_fwd(forth[i], op(lin_out[i]), B, Hh, Hh, op(xin[i]), pa_none(), forth_tmp[i], nullptr));
            TRY(conv_fwd(inc[i], pa_plain(heat64[i]), B, Hh, Hh, pa_plain(forth_tmp[i]), pa_none(), xin[i + 1].raw, nullptr));
        }
    }
    if (pts) TRY(pa_launch_loss_out(loss_dev, loss_keep, loss_out_dev, loss_total_out, stacks, st));
    return 0;
}

// hand-written backward of the whole pose net; gradients land in the flat `grads` array
int Net::backward_stack(int i) {
    const int Hh = res / 4;
    const float gscale = PA_GRAD_SCALE / ((float)B * 16.f * (float)Hh * (float)Hh);      // (fp16 build: scaled gradients, common.h)
    const bool inner = i + 1 < stacks;
    if (inner) {
        const PaOperand gx = pa_plain(xin[i + 1].grad);
        TRY(conv_wgrad(inc[i], gx, pa_plain(heat64[i]), B, Hh, Hh));
        TRY(conv_dgrad(inc[i], gx, B, Hh, Hh, pa_none(), pa_none(), ep_plain(), dheat_in[i]));
        TRY(conv_wgrad(forth[i], gx, op(lin_out[i]), B, Hh, Hh));
    }
    const bf16* din = inner ? dheat_in[i] : nullptr;
    if (heat_grads_on) {        // the caller's gradient (pa_hg_set_heat_grads), unscaled: only the half-precision build's PA_GRAD_SCALE is applied
        TRY(account(pa_work_heat_inject(elems(B, Hh, Hh, 1), heat_grads[i] != nullptr, inner),
                    [&] { return pa_launch_heat_inject(heat_grads[i], heat_grads_layout, din, dheat64[i], PA_GRAD_SCALE, B, Hh, Hh, st); }));
    } else {
        TRY(account(pa_work_heat_grad(elems(B, Hh, Hh, 1), inner), [&] { return pa_launch_heat_grad(heat[i], pts_dev, din, dheat64[i], gscale, B, Hh, Hh, st); }));
    }
    const PaOperand gh = pa_plain(dheat64[i]);
    TRY(conv_wgrad(outc[i], gh, op(lin_out[i]), B, Hh, Hh));
    if (inner) {
        TRY(conv_dgrad(outc[i], gh, B, Hh, Hh, pa_none(), pa_none(), ep_plain(), lgrad_tmp[i]));
        TRY(conv_dgrad(forth[i], pa_plain(xin[i + 1].grad), B, Hh, Hh, pa_plain(lgrad_tmp[i]), pa_none(),
                       final_ep(lin_out[i]), lin_out[i].grad));
    } else {
        TRY(conv_dgrad(outc[i], gh, B, Hh, Hh, pa_none(), pa_none(), final_ep(lin_out[i]), lin_out[i].grad));
    }
    TRY(finish_grad(lin_out[i]));
    PaOperand gl = gradop(lin_out[i]);
    bool gl_stored = false;                  // lgrad_tmp[i] is free again: the data gradient stores dz there for the weight gradient
    TRY(conv_dgrad(lin[i], gl, B, Hh, Hh, pa_none(), pa_none(), final_ep(post[i].out()), post[i].out().grad, lgrad_tmp[i], &gl_stored));
    if (gl_stored) gl = pa_plain(lgrad_tmp[i]);
    TRY(conv_wgrad(lin[i], gl, op(post[i].out()), B, Hh, Hh));
    TRY(finish_grad(post[i].out()));
    post[i].head().low_of_in = hg[i].low_fusable(*this, 0) ? &hg[i].up[0].out() : nullptr;          // (post_res reads merged[0]: its conv1 data gradient can emit d up1 too)
    TRY(post[i].bwd(*this, hg[i].out(), pa_none(), true));
    hg[i].low_done[0] = post[i].head().low_fused;
    TRY(hg[i].bwd(*this, xin[i], inner ? pa_plain(xin[i + 1].grad) : pa_none()));
    return 0;
}

// stem: residual3 <- residual2 <- maxpool <- residual1 <- 7x7 conv
int Net::backward_stem() {
    TRY(res3.bwd(*this, res2.x3, pa_none(), true));
    TRY(finish_grad(res2.x3));
    TRY(res2.bwd(*this, pool0, pa_none(), true));
    // the stem's pool: a launch that routes d pool0 into residual1's whole (four times larger) gradient -- or, routed, the launch's reductions
    // from a quarter of its input, and the routed gradient formed on load by its one reader, conv3's data gradient (which stores dz3 for the rest)
    stem_routed = stem_route_ok();
    res1.g3_pool_on = stem_routed;
    if (stem_routed) {
        TRY(account(pa_work_pool_stats(elems(B, res / 4, res / 4, 128)),
                    [&] { return pa_launch_maxpool_bwd_stats(pool0.grad, stem_xmax, op(res1.x3), final_ep(res1.x3), B, res / 2, res / 2, 128, st); }));
        TRY(finish_grad(res1.x3));
        res1.g3_pool = gradop(res1.x3);
        res1.g3_pool.mode = PA_LD_POOL; res1.g3_pool.p = pool0.grad; res1.g3_pool.map = stem_map;
        res1.g3_pool_ep = final_ep(res1.x3);
    } else {
        TRY(c_maxpool_bwd(*this, pool0.grad, op(res1.x3), pa_none(), final_ep(res1.x3), res1.x3.grad, B, res / 2, res / 2, 128, st));
        TRY(finish_grad(res1.x3));
    }
    TRY(res1.bwd(*this, a0, pa_none(), true));
    res1.g3_pool_on = false;
    TRY(finish_grad(a0));
    TRY(conv_wgrad(stem_conv, gradop(a0), pa_plain(cur_image), B, res / 2, res / 2));
    if (image_grad) {       // d loss / d image (pa_hg_set_image_grad): the same operand through the transposed 7x7/2 taps, untimed, on the main stream
        PaStemDgradArgs d; memset(&d, 0, sizeof d);
        d.g = gradop(a0); d.wf = stem_conv.wf; d.out = image_grad; d.B = B; d.Hm = res / 2; d.Wm = res / 2; d.layout = image_grad_layout;
        d.scale = 1.f / PA_GRAD_SCALE;
        TRY(account(pa_work_stem_dgrad(wop(d.g), B, d.Hm, d.Wm, d.layout), [&] { return pa_launch_stem_dgrad(d, st); }));
    }
    TRY(reduce_grads());
    return join_meters();               // the step's meters ran beside this pass: later readers on the main stream come behind them
}

// both halves of the stem's routed pool exist for this shape: the statistics launch (the streaming plans of the pool) and the pool-routed load
// of residual1's conv3 data gradient, which must also be the launch that stores dz3 for the later readers of that gradient
bool Net::stem_route_ok() {
    if (!(pool_route & 2) || !stem_map_written || ablated(PA_L_STEM_ROUTE)) return false;
    const int H = res / 2;
    if (!pa_pool_stats_route_supported(op(res1.x3), final_ep(res1.x3), B, H, H, 128)) return false;
    const PaEpilogue mask = final_ep(res1.x3); PaConvShape s{};
    s.B = B; s.H = H; s.W = H; s.Cin = res1.c3.pcout; s.Cout = res1.c3.pcin; s.taps = res1.c3.taps(); s.cus = pa_conv_cus();
    s.in_mode = PA_LD_POOL; s.in_map = stem_map != nullptr; s.in_q = gradop(res1.x3).q != nullptr; s.want_dz = res1.dz3 != nullptr;
    s.add1_mode = s.add2_mode = PA_LD_NONE; s.ep_mode = final_ep(res1.x2).mode; s.ep2_affine = mask.scale && mask.shift;
    return pa_conv_plan(s).pool_in;
}

int Net::fill_stem_grad() {
    return pa_launch_maxpool_bwd(pool0.grad, op(res1.x3), pa_none(), final_ep(res1.x3), res1.x3.grad, B, res / 2, res / 2, 128, st);
}

int Net::backward_pose() {
    TRY(ensure_streams());
    for (int i = stacks - 1; i >= 0; --i) TRY(backward_stack(i));
    return backward_stem();
}

// every gradient of hourglass `stack` is final once the main chain has enqueued its backward pass (the side branches are joined
// inside it) AND the weight-gradient stream has reduced its slabs: an event on that stream behind one on the main stream
int Net::mark_bucket(int stack) {
    if (stack < 0 || stack >= 16) return 1;
    if (!bucket_events) {
        for (int i = 0; i < 16; ++i) PA_CHECK(hipEventCreateWithFlags(&ev_bucket[i], hipEventDisableTiming));
        PA_CHECK(hipEventCreateWithFlags(&ev_bucket_main, hipEventDisableTiming));
        bucket_events = true;
    }
    TRY(flush_wgrads());
    if (!wgrads_aside()) return -1;            // slabs are only reduced at the very end in this mode: no early bucket
    TRY(flush_red_stash(wstream));
    PA_CHECK(hipEventRecord(ev_bucket_main, st));
    PA_CHECK(hipStreamWaitEvent(wstream, ev_bucket_main, 0));
    PA_CHECK(hipEventRecord(ev_bucket[stack], wstream));
    return 0;
}

// One training step (forward, loss, backward) as a HIP graph.  Inputs live in the engine's own buffers (img4, pts_dev:
// the caller copies into them on `st` before the launch), every pointer and shape inside is fixed by the layout, so the
// graph is captured once per (mode, bound memory) and replayed.  The capture runs the normal enqueue code: the side streams
// fork from / join into `st` by events, which the capture turns into graph dependencies.
int Net::train_step_graph(bool train) {
    TRY(ensure_streams());
    const int key = (train ? 1 : 0) | (multi_stream ? 2 : 0);
    if (drop_mask || prof.on) { pa_set_error_msg("train_step_graph: not with the occlusion branch / the launch profiler"); return 1; }
    // meters left on the meter stream by an eager step (pa_net_meters_async) read the heat maps / joints this launch overwrites; the
    // join must also happen OUTSIDE a capture (its event was recorded outside)
    TRY(join_meters());
    // (a replayed launch would carry the launch number of the capture: its barrier tags would match the previous replay's granules)
    if (!step_exec || step_key != key) {
        release_graph();
        // the caller's stream may be the legacy default stream, which cannot capture: capture on a stream of our own
        hipStream_t cap = nullptr, caller = st;
        PA_CHECK(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
        st = cap;
        hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeRelaxed);
        capturing = e == hipSuccess;          // (extension launches -- any-order weight gradients -- stay out of a capture)
        if (e != hipSuccess) { st = caller; (void)hipStreamDestroy(cap); pa_set_error("hipStreamBeginCapture", e, __FILE__, __LINE__); return (int)e; }
        int rc = forward_pose(nullptr, img4, pts_dev, train, nullptr);
        if (!rc) rc = backward_pose();
        hipGraph_t g = nullptr;
        e = hipStreamEndCapture(cap, &g);
        capturing = false;
        st = caller;
        (void)hipStreamDestroy(cap);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess) { pa_set_error("hipStreamEndCapture", e, __FILE__, __LINE__); return (int)e; }
        step_graph = g;
        PA_CHECK(hipGraphInstantiate(&step_exec, step_graph, nullptr, nullptr, 0));
        step_key = key;
    }
    train_bn = train;
    cur_image = img4;
    heat_peak_valid.assign(stacks, 0);
    PA_CHECK(hipGraphLaunch(step_exec, st));
    return 0;
}

void Net::release_graph() {
    if (step_exec) { (void)hipGraphExecDestroy(step_exec); step_exec = nullptr; }
    if (step_graph) { (void)hipGraphDestroy(step_graph); step_graph = nullptr; }
    step_key = -1;
}

int Net::reduce_grads() {
    TRY(flush_wgrads());
    if (wgrads_aside()) {                       // every slab is summed on the weight-gradient stream: the main stream waits for it
        TRY(flush_red_stash(wstream));
        PA_CHECK(hipEventRecord(ev_wdone, wstream));
        PA_CHECK(hipStreamWaitEvent(st, ev_wdone, 0));
        return 0;
    }
    TRY(pa_launch_wgrad_reduce(red_jobs, n_red, red_max, st));
    if (!is_agent) {
        TRY(pa_launch_stem_wgrad_reduce(stem_conv.part, stem_conv.splits, grads + stem_conv.p_w, st, grads + stem_conv.p_b));
    }
    return 0;
}
