// What a launch of the net COSTS, from what it IS: host-only pure functions, nothing from HIP (modes.h integers, like conv_plan.h).
// Two ledgers per launch, different on purpose:
//   rd / wr       DESIGN bytes (pa_net_design_bytes): every operand at its storage width, PADDED channels, the second operand of a BatchNorm-
//                 backward load, reference tensors of masked epilogues, stored dz, fp32 slabs written and read back, weights
//   bytes / flops ALGORITHMIC work of the event profile (pa_net_profile_report), convolutions only: every activation element once (2 bytes,
//                 REAL channels), weights once, 2 * M * N * K flops.  The stem's image counts 4-channel padded in both.
// tests/test_gpu_work_ledger.py pins both for whole steps: a change of what a launch reads or writes edits ONE function here.
#pragma once
#include "modes.h"

// classes of the event profile.  0-5: maps of >= PA_PROF_LOW_M pixels (32 x 32 and larger at batch 24: bandwidth- / MFMA-shaped launches);
// 9-11: every convolution below that (bound by launch / staging / epilogue LATENCY, DESIGN.md section 4: averaging them into the classes
// above says nothing about either); PA_PROF_LOWRES_FWD: unused slot (a launch removed in round 4) -- the indices are public
enum { PA_PROF_FWD1 = 0, PA_PROF_FWD3, PA_PROF_DGRAD1, PA_PROF_DGRAD3, PA_PROF_WGRAD1, PA_PROF_WGRAD3, PA_PROF_STEM_FWD,
       PA_PROF_STEM_WGRAD, PA_PROF_LOWRES_FWD, PA_PROF_LOW_FWD, PA_PROF_LOW_DGRAD, PA_PROF_LOW_WGRAD, PA_PROF_NCLS };
#define PA_PROF_LOW_M 16384

struct PaWork { double rd, wr;            // design bytes (pa_net_design_bytes)
                double bytes, flops;      // algorithmic work of the event profile
                int cls; };               // PA_PROF_* (or -1: not a profiled launch)
struct PaWorkOp { int mode; bool q; };      // an operand as the ledgers see it: load mode; a pool-routed one may carry a plain addend q
// a convolution layer at one map: real and padded channels, kernel size (7: the stem, a K = 256 GEMM over the 4-channel image), slabs
struct PaWorkConv {
    int B, H, W, cin, cout, pcin, pcout, k, splits;
    double M() const { return (double)B * H * W; }
    double taps() const { return k == 7 ? 1 : k * k; }
    double image() const { return 2.0 * B * 4.0 * H * W * 4; }      // the stem's input, read once
};

inline double pa_work_opb(PaWorkOp o, double elems) {      // design bytes of one operand
    if (o.mode == PA_LD_POOL) return (2.0 + 1.0) * elems / 4 + (o.q ? 2.0 * elems : 0.0);      // pooled gradient + byte map, plain addend
    return o.mode == PA_LD_NONE ? 0.0 : (o.mode == PA_LD_LIN2 ? 4.0 : 2.0) * elems;
}
inline PaWork pa_work_stream(double rd, double wr) { return PaWork{rd, wr, 0.0, 0.0, -1}; }      // a streaming launch: design bytes only

// the profile's half of a convolution launch; direction: 0 forward, 1 data gradient, 2 weight gradient (fp32 weights)
inline PaWork pa_work_conv_profile(const PaWorkConv& c, int direction) {
    const bool stem = c.k == 7;
    const double cin = stem ? 147 : c.cin, wbytes = (direction == 2 ? 4.0 : 2.0) * c.cout * c.taps() * cin;
    const int big[3][2] = {{PA_PROF_FWD1, PA_PROF_FWD3}, {PA_PROF_DGRAD1, PA_PROF_DGRAD3}, {PA_PROF_WGRAD1, PA_PROF_WGRAD3}};
    PaWork w{};
    w.bytes = (stem ? c.image() + 2.0 * c.M() * 64 : 2.0 * c.M() * (cin + c.cout)) + wbytes;
    w.flops = 2.0 * c.M() * c.cout * c.taps() * cin;
    w.cls = stem ? (direction == 2 ? PA_PROF_STEM_WGRAD : PA_PROF_STEM_FWD) : c.M() < PA_PROF_LOW_M ? PA_PROF_LOW_FWD + direction : big[direction][c.k == 3];
    return w;
}
inline PaWork pa_work_conv_fwd(const PaWorkConv& c, PaWorkOp in, PaWorkOp add1, PaWorkOp add2) {
    PaWork w = pa_work_conv_profile(c, 0);
    w.rd = (c.k == 7 ? c.image() : pa_work_opb(in, c.M() * c.pcin)) + pa_work_opb(add1, c.M() * c.pcout) + pa_work_opb(add2, c.M() * c.pcout)
         + 2.0 * c.pcout * c.taps() * c.pcin;
    w.wr = 2.0 * c.M() * c.pcout;
    return w;
}
// data gradient: the GEMM runs from the layer's (padded) outputs to its inputs.  stores_dz: PaConvPlan::stores_dz; row_up: the plan is
// PA_CVP_ROW_UP (the launch also emits the low-resolution half of the upsample-add backward: a quarter of its output more, read and written)
inline PaWork pa_work_conv_dgrad(const PaWorkConv& c, PaWorkOp dy, PaWorkOp add1, PaWorkOp add2, int ep_mode, bool stores_dz, bool row_up) {
    PaWork w = pa_work_conv_profile(c, 1);
    const double in = c.M() * c.pcout, out = c.M() * c.pcin, wbytes = 2.0 * c.pcin * c.taps() * c.pcout;
    if (dy.mode == PA_LD_POOL) { w.rd = pa_work_opb(dy, in) + 2.0 * out + wbytes; w.wr = 2.0 * out + 2.0 * in; return w; }
    w.rd = pa_work_opb(dy, in) + pa_work_opb(add1, out) + pa_work_opb(add2, out) + (ep_mode == PA_OUT_BWD ? 2.0 * out : 0.0) + wbytes + (row_up ? 2.0 * out / 4 : 0.0);
    w.wr = 2.0 * out + (stores_dz ? 2.0 * in : 0.0) + (row_up ? 2.0 * out / 4 : 0.0);
    return w;
}
inline PaWork pa_work_conv_wgrad(const PaWorkConv& c, PaWorkOp dy, PaWorkOp x) {      // slabs written, read back by the reducer, gradient written
    PaWork w = pa_work_conv_profile(c, 2);
    const double slab = 4.0 * c.splits * c.pcout * c.taps() * c.pcin;
    w.rd = (c.k == 7 ? c.image() : pa_work_opb(x, c.M() * c.pcin)) + pa_work_opb(dy, c.M() * c.pcout) + slab;
    w.wr = slab + 4.0 * c.pcout * c.taps() * c.pcin;
    return w;
}
// ---- the streaming launches; e: elements of the FULL-resolution tensor (B * H * W * C)
inline PaWork pa_work_maxpool_fwd(PaWorkOp in, double e, bool map, bool xmax) {
    return pa_work_stream(pa_work_opb(in, e), 2.0 * e / 4 + (map ? e / 4 : 0.0) + (xmax ? 2.0 * e / 4 : 0.0));
}
inline PaWork pa_work_maxpool_bwd(PaWorkOp in, PaWorkOp add, int ep_mode, double e) {
    return pa_work_stream(2.0 * e / 4 + pa_work_opb(in, e) + pa_work_opb(add, e) + (ep_mode == PA_OUT_BWD ? 2.0 * e : 0.0), 2.0 * e);
}
inline PaWork pa_work_pool_stats(double pooled) { return pa_work_stream(4.0 * pooled, 0.0); }      // the routed pool's statistics launch: gradient + arg-max value, POOLED elements
inline PaWork pa_work_upadd_fwd(PaWorkOp low, PaWorkOp skip, double e) { return pa_work_stream(pa_work_opb(low, e / 4) + pa_work_opb(skip, e), 2.0 * e); }
inline PaWork pa_work_upadd_bwd(double e, int part, int ep_low_mode, int ep_skip_mode) {      // part: bit 0 the low-resolution output, bit 1 the skip output
    return pa_work_stream(2.0 * e + ((part & 1) && ep_low_mode == PA_OUT_BWD ? 2.0 * e / 4 : 0.0) + ((part & 2) && ep_skip_mode == PA_OUT_BWD ? 2.0 * e : 0.0),
                          ((part & 1) ? 2.0 * e / 4 : 0.0) + ((part & 2) ? 2.0 * e : 0.0));
}
// ---- head and loss; M: pixels of the heat maps (B * res/4 * res/4)
inline PaWork pa_work_head_fwd(PaWorkOp x, double M, int chan) { return pa_work_stream(pa_work_opb(x, M * chan) + 2.0 * 16 * chan, M * 16 * 4 + M * 64 * 2); }
inline PaWork pa_work_heat_grad(double M, bool din) { return pa_work_stream(M * 16 * 4 + (din ? M * 64 * 2 : 0.0), M * 64 * 2); }
inline PaWork pa_work_heat_inject(double M, bool G, bool din) { return pa_work_stream((G ? M * 16 * 4 : 0.0) + (din ? M * 64 * 2 : 0.0), M * 64 * 2); }
// the stem's data gradient: g over the B x Hm x Wm x 64 stem output, fp32 image gradient out (layout 1: 4 floats per pixel, 0: 3)
inline PaWork pa_work_stem_dgrad(PaWorkOp g, int B, int Hm, int Wm, int layout) {
    return pa_work_stream(pa_work_opb(g, (double)B * Hm * Wm * 64) + 2.0 * 64 * 256, 4.0 * B * (2 * Hm) * (2 * Wm) * (layout ? 4 : 3));
}
