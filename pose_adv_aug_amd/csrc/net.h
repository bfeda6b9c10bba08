// Stacked-hourglass pose network + ASN scale/rotation agent as an explicit launch plan over the
// HIP kernels (no autograd, no graph compiler): forward saves exactly what the hand-written backward
// needs.  Mirrors the reference module tree (models/asn_stacked_hg.py) name-for-name so that
// checkpoints interchange.  Internal header; the public C ABI is include/poseadv.h.
#pragma once
#include <string.h>
#include <string>
#include <vector>
#include "common.h"
#include "kernels.h"
#include "pose_ops.h"
#include "work_model.h"

#define TRY(x) do { int _r = (x); if (_r) return _r; } while (0)
inline PaEpilogue ep_plain() { PaEpilogue e; memset(&e, 0, sizeof e); e.mode = PA_OUT_PLAIN; return e; }

struct Arena {
    char* base = nullptr;
    size_t off = 0;
    void* take(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
    template <typename T> T* get(size_t n) { return reinterpret_cast<T*>(take(n * sizeof(T))); }
};

struct TensorInfo {          // one state_dict entry
    std::string name;
    int shape[4];
    int ndim;
    size_t offset;           // element offset into the flat parameter (or buffer) array
    size_t numel;
    int is_buffer;           // 0 parameter, 1 running_mean/var buffer, 2 num_batches_tracked (host-side int64)
};

struct BNLayer {
    int C = 0;
    size_t p_gamma = 0, p_beta = 0, b_rmean = 0, b_rvar = 0;
    float *stats = nullptr, *bstats = nullptr;                 // partial rows [rows][C][2] (forward stats / backward reductions)
    int stat_rows = 0, bstat_rows = 0, max_rows = 0;
    float *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;
    float *kA = nullptr, *kB = nullptr, *kC = nullptr;
    // the finalize of the forward statistics / of the backward reductions has NOT been launched: the next consumer of the tensor does it
    // in its prologue (bn_fin.h; Net::fin_rows_max)
    bool fin_pending = false, bfin_pending = false;
};

struct ConvLayer {
    int Cin = 0, Cout = 0, k = 1;          // real dims
    int pcin = 0, pcout = 0;               // padded (multiple of 64) dims used by the kernels
    size_t p_w = 0, p_b = 0;
    bf16 *wf = nullptr, *wb = nullptr;
    float *part = nullptr, *dbpart = nullptr;
    int splits = 0;
    int red_index = -1;                    // index of this layer's job in the reduce table
    size_t part_floats = 0, db_floats = 0;
    bool has_bn_after = true;
    int taps() const { return k * k; }
};

struct Act {                 // NHWC bf16 activation; `bn` != null means BatchNorm+ReLU is still pending
    bf16* raw = nullptr;
    bf16* grad = nullptr;    // masked gradient dz when bn != null, plain gradient otherwise
    BNLayer* bn = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    size_t numel() const { return (size_t)B * H * W * C; }
    int M() const { return B * H * W; }
};

struct Net;

// optional per-launch timing of the MFMA kernels with HIP events (bench.py's roofline object); the classes: work_model.h
struct ProfEntry { hipEvent_t e0, e1; int cls; double bytes, flops; };
struct Prof {
    bool on = false;
    std::vector<ProfEntry> entries;
    size_t used = 0;
    std::vector<int> last_seq;            // class of every launch of the last reported pass, in launch order
    ProfEntry* begin(int cls, double bytes, double flops, hipStream_t st);
    void end(ProfEntry* e, hipStream_t st);
    int report(double* out /* [PA_PROF_NCLS][4] = total ms, launches, algorithmic bytes, flops */);
};

struct Residual {
    ConvLayer c1, c2, c3, ad;
    BNLayer b1, b2, b3;
    bool has_adapter = false;
    int cin = 0, cout = 0;
    Act x1, x2, x3;          // raw conv outputs (x3 includes the shortcut)
    bf16* adout = nullptr;   // adapter(x)
    bf16* adgrad = nullptr;  // scratch for the adapter's data gradient
    bf16* dz3 = nullptr;     // BatchNorm-backward gradient of x3, materialised by conv3's data gradient for its later consumers
    bool dz3_valid = false;
    bf16* dz2 = nullptr;     // the same for x2 (stored by conv2's data gradient, read by conv2's weight gradient)
    bool dz2_valid = false;
    void declare(Net& n, const std::string& prefix, int cin, int cout, bool adapter);
    void layout(Net& n, Arena& a, int B, int H, int W, bool need_grad);
    int fwd(Net& n, const Act& in);
    int bwd(Net& n, const Act& in, const PaOperand& extra, bool in_needs_grad);
    // round 6: `in` is the upsample-add output merged[k] of an hourglass and low_of_in the low-resolution tensor up[k].x3 under it -- conv1's data
    // gradient (which produces d merged) then also emits d up[k].x3 (2 x 2 sums, mask, reductions) where its tile kernel can
    // (Net::conv_dgrad / conv_plan.h: PA_CVP_ROW_UP); low_fused says whether it did
    const Act* low_of_in = nullptr;
    bool low_fused = false;
    // the gradient of x3 arrives pool-routed (Net::stem_route_ok): conv3's data gradient forms dz from g3_pool (PA_LD_POOL) and g3_pool_ep's mask
    bool g3_pool_on = false; PaOperand g3_pool; PaEpilogue g3_pool_ep;
    int b3_rows_scale = 1;   // partial-row capacity of bn3's backward reductions in units of this block's own map (4: the rows may come from a launch over the 2x larger map)
    int bwd_a(Net& n, const Act& in);                                  // everything except the input gradient
    int bwd_b(Net& n, const Act& in, const PaOperand& extra);           // input gradient (needs `extra`)
};

// One site of the reference's module tree: nn.Sequential of num_modules residual blocks (reference :73-77, :272-276).  Block j reads block
// j-1's x3 (pending BatchNorm, two readers: conv1 and conv3's shortcut addend).  What a site does towards its neighbours splits between the two
// ends: head() carries the input side (low_of_in / low_fused, the `extra` addend of the input gradient), tail() the output side (out(),
// b3_rows_scale, the target of a fused low-resolution gradient).  Sized once in declare(): the layers register pointers into Net::convs / bns.
struct Chain {
    std::vector<Residual> m;
    Residual& head() { return m.front(); }
    Residual& tail() { return m.back(); }
    const Residual& tail() const { return m.back(); }
    const Act& out() const { return m.back().x3; }
    const Act& tail_in(const Act& in) const { return m.size() > 1 ? m[m.size() - 2].x3 : in; }      // what the last block reads
    void declare(Net& n, const std::string& site_prefix, int chan, int modules);      // "<site_prefix><j>." per block
    void layout(Net& n, Arena& a, int B, int H, int W, bool need_grad, int tail_b3_rows_scale = 1);
    int fwd(Net& n, const Act& in);
    // precondition as Residual::bwd, on the last block.  bwd_a: everything except the first block's input gradient; bwd_b: that gradient
    int bwd_a(Net& n, const Act& in);
    int bwd_b(Net& n, const Act& in, const PaOperand& extra) { return m.front().bwd_b(n, in, extra); }
    int bwd(Net& n, const Act& in, const PaOperand& extra, bool in_needs_grad);
};

struct Hourglass {
    Chain down[4], up[4], skip[4], neck;
    Act pooled[4], merged[4];     // pool outputs p_k (k=1..4), upsample-add outputs o_k
    Act skipm[4], neckm;          // occlusion branch only: skip / neck outputs times the 4x4 cell mask (reference :79-100)
    bf16* poolgrad[4] = {nullptr, nullptr, nullptr, nullptr};   // gradient of the pool routed back to its input
    bool low_done[4] = {false, false, false, false};             // d up[k].x3 of this backward pass came out of the data gradient that produced d merged[k]
    // pool routing (Net::pool_route): the forward pool k also stores its arg-max byte map, and the first block of skip[k] reads the pool's
    // gradient through it (PA_LD_POOL) -- no pool backward launch, poolgrad[k] is only filled on request (fill_poolgrad: the debug view)
    unsigned char* poolmap[4] = {nullptr, nullptr, nullptr, nullptr};
    bool map_written[4] = {false, false, false, false};          // by the last forward pass
    bool routed[4] = {false, false, false, false};               // the last backward pass routed pool k: poolgrad[k] is stale
    PaOperand route_extra[4];                                    // ... and this was its plain addend (extra0 at k = 0)
    bool route_ok(Net& n, int k, const Act& x, const PaOperand& ex0);
    int fill_poolgrad(Net& n, int k, const Act& in);             // run the pool backward launch of a routed level into poolgrad[k]
    void declare(Net& n, const std::string& prefix, int chan);
    void layout(Net& n, Arena& a, int B, int H, int W, bool need_grad);
    int encode(Net& n, const Act& in);
    int decode(Net& n);
    int bwd(Net& n, const Act& in, const PaOperand& extra0);
    const Act& out() const { return merged[0]; }
    bool low_fusable(const Net& n, int k) const;     // may the producer of d merged[k] also emit d up[k].x3 (the skip half then needs the one-output launch)
};

struct Net {
    // configuration
    int stacks = 2, modules = 1, chan = 256, classes = 16, B = 0, res = 256;
    bool is_agent = false;
    // tables
    std::vector<TensorInfo> tensors;           // state_dict order
    size_t n_params = 0, n_buffers = 0;
    std::vector<ConvLayer*> convs;
    std::vector<BNLayer*> bns;
    // bound memory
    float *params = nullptr, *grads = nullptr, *buffers = nullptr;
    char* workspace = nullptr;
    size_t workspace_bytes = 0;
    float *stats_arena = nullptr;
    size_t stats_arena_floats = 0;
    float* loss_dev = nullptr;                 // [stacks] per-stack loss accumulators (atomics of head_fwd), part of the stats arena
    float* loss_keep = nullptr;                // [stacks + 1] the last pose forward pass's losses and their sum (loss_out_kernel)
    float* loss_total_out = nullptr;           // caller's device float that also receives the sum (pa_hg_set_loss_total), or NULL
    bool loss_self_clearing = false;           // pose nets: the accumulators are cleared by loss_out_kernel, begin_step() skips its memset
    // device job tables
    PaPrepJob* prep_jobs = nullptr; int n_prep = 0, prep_max = 0;
    PaWgradReduceJob* red_jobs = nullptr; int n_red = 0, red_max = 0;
    PaBnEvalJob* bneval_jobs = nullptr; int n_bneval = 0;
    // run state
    hipStream_t st = nullptr;
    // side stream: the skip branch of every hourglass level runs on `side` next to the low-resolution path (tiny, latency-bound kernels
    // that leave most CUs idle); fork / join by one event pair per level, joined before the call returns.  ONE stream for all four skip
    // branches: main + side + weight-gradient stream = 3 hardware queues (the runtime has 4)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork[4], ev_join[4];
    bool streams_ready = false, multi_stream = !pa_tuning().single_stream;
    // weight-gradient launches only feed the slab reducer: they run on their own stream behind an event recorded where their operands
    // are final, off the dgrad / BatchNorm critical chain
    hipStream_t wstream = nullptr;
    bool wgrads_aside() const { return multi_stream && wstream != nullptr; }      // the weight gradients run on wstream
    hipEvent_t ev_w[16]; int ev_w_next = 0;
    hipEvent_t ev_wdone;
    // weight-gradient launches are collected and flushed in groups: ONE event record on the producing stream per group
    // (an event record between two kernels of a queue costs a 15-20 us bubble on it: ~100 records per step were 1.5 ms)
    struct PendingWgrad { PaWgradArgs a; PaWork w; bool stem; int job_wgs; ConvLayer* c; };      // job_wgs: workgroups as a job of a group launch (0: launched alone)
    // with a weight-gradient stream, the slabs of a group are summed right behind it on that stream (part of them still in the 256 MB
    // Infinity Cache) instead of by one 280 us reduction on the main stream at the end of the step
    std::vector<PendingWgrad> pending_wgrads;
    bool on_side = false;                      // the launches being enqueued belong to a side branch (StreamScope)
    int flush_wgrads();                        // record on `st`, make wstream wait, launch the collected weight gradients
    int launch_pending_wgrads();               // its body; flush_wgrads() empties the list (and on an error the stash) behind it
    std::vector<int> red_stash; int red_stash_mx = 0, red_stash_flushes = 0;      // reduce-table indices of flushed layers whose slabs are not summed yet
    int flush_red_stash(hipStream_t ws);       // one reduction launch for the stash
    void drop_wgrads();                        // error exits: forget the collected launches and the stash
    int ensure_streams();
    void release_streams();                    // destroys the side streams / events (pa_net_destroy)
    int fork_to(int k);                        // level k's branch on the side stream waits for everything enqueued on st so far
    int record_join(int k);                    // mark the end of that branch
    int wait_join(int k);                      // st waits for that mark
    Prof prof;
    // bytes this design moves (pa_net_design_bytes): operands of every launch since begin_step(), counted once per launch (work_model.h)
    double dbytes_rd = 0, dbytes_wr = 0;
    void cnt(const PaWork& w) { dbytes_rd += w.rd; dbytes_wr += w.wr; }
    // PA_ABLATE (tuning builds; constant false in the release build): is this launch left out?  kind: PA_L_*, the table of the bits in net.hip
    bool ablated(int kind, int k = 0, int H = 1 << 30, long M = 0) const;
    // ONE launch: its design bytes counted, its profile entry (w.cls >= 0) around launch() on `st`.  skip: the instrument leaves the launch
    // out (the entry stays, 0 is returned) -- its bytes are then counted only where count_skipped says the site always did
    template <class F> int account(const PaWork& w, F launch, bool skip = false, bool count_skipped = true);
    // forward + loss + backward of the training step captured ONCE into a HIP graph (fork / join events of the side and
    // weight-gradient streams become graph edges) and replayed: pa_hg_train_step with use_graph
    hipGraph_t step_graph = nullptr; hipGraphExec_t step_exec = nullptr; int step_key = -1;
    int train_step_graph(bool train);
    void release_graph();
    bool train_bn = true;
    int bn_update = 1;                         // 0: use batch statistics without touching the running estimates
    float momentum = 0.1f, eps = 1e-5f;

    // ---- pose net modules
    ConvLayer stem_conv; BNLayer stem_bn;
    Residual res1, res2, res3;
    std::vector<Hourglass> hg;
    std::vector<Chain> post;
    std::vector<ConvLayer> lin; std::vector<BNLayer> lin_bn;
    std::vector<ConvLayer> outc, forth, inc;
    bf16* img4 = nullptr;
    Act a0, pool0;
    std::vector<Act> lin_out, xin;                 // xin[i] = input of stack i
    std::vector<float*> heat; std::vector<bf16*> heat64, dheat64, dheat_in, forth_tmp, lgrad_tmp;
    double* pts_dev = nullptr;                     // [B][16][2] heat-map coords (caller provided per step)
    std::vector<float*> heat_peak;                 // [B][16][2] arg-max of heat[i], computed once per forward on demand (accuracy AND PCKh use it)
    std::vector<char> heat_peak_valid;
    int heat_argmax(int stack, const float** out, hipStream_t on = nullptr); // launches the arg-max unless this forward's result exists
    // The meters of a training step (pa_hg_accuracy / pa_hg_pckh: ~8 short launches that only READ the forward pass's heat maps) on a stream of
    // their own beside the backward pass (pa_net_meters_async): forked behind the last launch of the main stream, joined by the main stream
    // at the end of the backward pass (or in front of the next forward pass), so every later reader on the main stream is ordered behind them.
    hipStream_t mstream = nullptr; hipEvent_t ev_mfork = nullptr, ev_meter = nullptr;
    bool meters_async = false, meter_pending = false;
    bool capturing = false;                     // inside train_step_graph's stream capture
    int meter_stream(hipStream_t* out);         // the stream the meters are launched on now (forks mstream from st when meters_async)
    int meter_done(hipStream_t ms);             // records the join event when ms is the meter stream
    int join_meters();                          // the main stream waits for the pending meters
    // occlusion (dropout) branch, reference :172-190: [B][16] cell masks (caller-owned device memory) applied to the neck and the
    // four skip tensors of every stack in forward_pose / backward_pose; nullptr = off
    const float* drop_mask = nullptr;
    // d loss / d heat given by the caller (pa_hg_set_heat_grads): while on, backward_stack(i) takes heat_grads[i] (caller-owned device
    // memory, nullptr = zero) through pa_launch_heat_inject instead of the built-in MSE gradient (heat_grad_kernel); pts_dev is not read
    std::vector<const float*> heat_grads;
    int heat_grads_layout = 0;                  // 0: [B][16][H][W], 1: [B][H*W][16]
    bool heat_grads_on = false;
    // d loss / d image wanted by the caller (pa_hg_set_image_grad): while set, backward_stem() also runs the stem's data gradient
    // (stem_dgrad.hip) into this caller-owned fp32 buffer, unscaled; nullptr = off, and the step is launch for launch what it is without
    float* image_grad = nullptr;
    int image_grad_layout = 0;                  // 0: [B][3][res][res], 1: [B][res][res][4]

    // ---- declaration helpers
    size_t add_param(const std::string& name, std::initializer_list<int> shape);
    size_t add_buffer(const std::string& name, int C);
    void declare_conv(ConvLayer& c, const std::string& name, int cin, int cout, int k, bool bn_after);
    void declare_bn(BNLayer& b, const std::string& name, int C);
    void layout_conv(ConvLayer& c, Arena& a, int M, int H = 0, int W = 0);
    void layout_bn(BNLayer& b, Arena& a, int M);
    Act new_act(Arena& a, int B, int H, int W, int C, BNLayer* bn, bool need_grad);

    void declare_pose();
    size_t layout_all(char* base);
    int upload_tables();

    // ---- runtime helpers
    PaOperand op(const Act& a) const;               // value of an activation (BNRELU pending or PLAIN)
    PaOperand gradop(const Act& a) const;           // gradient w.r.t. the raw tensor (LIN2 or PLAIN)
    PaEpilogue final_ep(const Act& a) const;        // epilogue that finishes a gradient for `a`
    int finish_grad(const Act& a);                  // BatchNorm backward finalize (if pending BN)
    int finish_grad2(const Act& a, const Act& b);   // two of them in one launch
    // pending_in: the BatchNorm of `in` whose finalize may still be pending (done in this launch's prologue then);
    // defer_after: the caller guarantees that the ONLY next reader of bn_after's constants is a launch that takes a pending finalize
    // (fin_consumer_ok), so the finalize launch is skipped when the statistics have <= fin_rows_max partial rows
    int conv_fwd(ConvLayer& c, const PaOperand& in, int B, int H, int W, const PaOperand& add1, const PaOperand& add2,
                 bf16* out, BNLayer* bn_after, BNLayer* pending_in = nullptr, bool defer_after = false);
    int conv_dgrad(ConvLayer& c, const PaOperand& dy, int B, int H, int W, const PaOperand& add1, const PaOperand& add2,
                   const PaEpilogue& ep, bf16* out, bf16* dz_out = nullptr, bool* dz_done = nullptr, BNLayer* pending_in = nullptr,
                   const Act* low = nullptr, bool* low_done = nullptr,      // low: also emit the upsample-add backward's low-resolution output (Residual::low_of_in)
                   const PaEpilogue* pool_in_ep = nullptr);                  // dy is pool-routed (PA_LD_POOL): the mask the pool backward launch would have applied
    // BatchNorm finalize in the consumer's prologue for launches with at most this many partial rows (the 16 x 16 and smaller levels;
    // 0 = always a launch of its own).  Same bits either way (bn_fin.h)
    int fin_rows_max = pa_tuning().fin_prologue > PA_FIN_SMALL_ROWS ? PA_FIN_SMALL_ROWS : pa_tuning().fin_prologue;
    int pool_route = pa_tuning().pool_route;            // pool gradients through the arg-max map: bit 0 the hourglass pools (Hourglass::poolmap), bit 1 the stem's (stem_map); pa_net_set_pool_route
    bool maps_on = false;                               // this forward pass stores the hourglass maps (a training pass of the whole net with pool_route & 1)
    // the stem's pool (residual1 -> pool0): map + the raw value at the arg-max; its backward pass is then a quarter-size statistics launch and
    // a pool-routed load in residual1's conv3 data gradient (Residual::g3_pool) instead of a launch that writes residual1's whole gradient
    unsigned char* stem_map = nullptr; bf16* stem_xmax = nullptr;
    bool stem_map_written = false, stem_routed = false;      // by the last forward pass / the last backward pass routed it: res1.x3.grad is stale
    bool stem_route_ok();
    int fill_stem_grad();                               // run the pool backward launch into res1.x3.grad (the debug view of a routed step)
    int fin_mask = pa_tuning().fin_mask;       // which finalizes may ride in a consumer: 1 forward x1 / x2, 2 backward x2, 4 backward x3
    bool fin_consumer_ok(const ConvLayer& c, int B, int H, int W, bool dgrad) const;
    PaBnFin fin_fwd(const BNLayer& b, int M) const;
    PaBnFin fin_bwd(const BNLayer& b, int M) const;
    bool fin_can_wait(const BNLayer* bn, bool defer, bool bwd) const {      // this BatchNorm's forward / backward finalize can wait for its consumer
        return bn && defer && (bwd ? bn->bstat_rows : bn->stat_rows) > 0 && (bwd ? bn->bstat_rows : bn->stat_rows) <= fin_rows_max;
    }
    int finish_grad_or_defer(const Act& a, bool defer);
    int finish_grad2_or_defer(const Act& a, bool defer_a, const Act& b, bool defer_b);
    bool x3_fin_ok(const Residual& r, const Act& in) const;     // can r.x3's backward finalize ride in conv3's data gradient?
    bool x3_fin_ok(const Chain& c, const Act& in) const { return x3_fin_ok(c.tail(), c.tail_in(in)); }      // the same for a chain's output
    int conv_wgrad(ConvLayer& c, const PaOperand& dy, const PaOperand& x, int B, int H, int W);

    int prepare_weights();
    int begin_step();
    const bf16* cur_image = nullptr;
    int forward_pose(const float* img_nchw, const bf16* img4_in, const double* pts, bool train, float* loss_out_dev);
    int forward_pose_body(const float* img_nchw, const bf16* img4_in, const double* pts, bool train, float* loss_out_dev);
    int backward_pose();
    // the backward pass in phases (data-parallel gradient exchange of a finished stack while the earlier ones still run):
    // phase p < stacks = head layers + post block + hourglass of stack (stacks-1-p); phase == stacks = stem + final reductions
    int backward_stack(int i);
    int backward_stem();
    hipEvent_t ev_bucket[16], ev_bucket_main = nullptr; bool bucket_events = false;
    int mark_bucket(int stack);                     // record "every gradient of hg.<stack> is final" (after its slabs are reduced)
    int reduce_grads();
    int forward_half(const float* img_nchw, const bf16* img4_in, bool train);     // stem + hg[0] down path (agent features)

    // ---- ASN scale/rotation agent (is_agent == true): reference models/asn_stacked_hg.py:349-439
    int scale_num = 7, rot_num = 7;
    Residual asn_in[5];                            // residual_skip1..4, residual_neck
    Residual asn_merge[4];
    Residual asn_deep[3];
    size_t p_fcs_w = 0, p_fcs_b = 0, p_fcr_w = 0, p_fcr_b = 0;
    Act asn_pa[4];                                 // maxpool(previous) + lower feature
    float *asn_feat = nullptr, *asn_logits = nullptr, *asn_probs = nullptr, *asn_dlogits = nullptr;   // [B][C], [B][2K] ...
    void declare_asn();
    size_t layout_asn(char* base);
    int asn_forward(Net& pose, bool train, float* logits_s, float* logits_r);
    float asn_log_eps = 1e-7f;                 // log(softmax + eps) of the agent's KL loss
    int asn_backward(Net& pose, const float* target_s, const float* target_r, float* loss_out);
    int asn_backward_trunk(Net& pose, const bf16* dact);     // from the gradient of deep_merge's output down to every trunk parameter
    // occlusion agent (create_asn(is_dropout=True), reference :378-379,437-439): out_conv 1x1 chan -> 1 on the 4x4 map
    bool asn_dropout = false;
    size_t p_oc_w = 0, p_oc_b = 0;
    int asn_forward_trunk(Net& pose, bool train, const Act** top);
    int asn_forward_masks(Net& pose, bool train, float* mask_logits);
    int asn_backward_masks(Net& pose, const float* dlogits);
};

PaOperand pa_plain(const bf16* p);
PaOperand pa_none();
