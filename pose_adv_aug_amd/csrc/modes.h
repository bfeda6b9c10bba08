// Operand load / epilogue modes: plain integers shared by the device code (common.h) and the host-only planner (conv_plan.h); nothing from HIP
#pragma once
// How an NHWC operand is turned into a value when it is loaded (per element, per channel c):
//   PLAIN : v = p[i]
//   BNRELU: v = max(0, k0[c] * p[i] + k1[c])          (train/eval BatchNorm + ReLU applied on load)
//   LIN2  : v = k0[c] * p[i] + k1[c] * q[i] + k2[c]    (BatchNorm backward applied on load:
//                                                       p = masked upstream grad, q = raw conv output)
//   POOL  : (second epilogue addend of the 1x1 data gradients that have an instance for it only: PaConvPlan::pool_route) the gradient
//           of a 2x2 max pool routed to its arg-max through the byte map the forward pool stored, plus an optional plain addend q:
//           v = bf16((map[low(i)][c] == pos(i) ? p[low(i)][c] : 0) + q[i])   -- what maxpool_bwd would have stored at i
//           (p: gradient of the pooled tensor, low(i) the pooled pixel over pixel i, pos(i) = 2 * (row & 1) + (column & 1))
enum { PA_LD_NONE = -1, PA_LD_PLAIN = 0, PA_LD_BNRELU = 1, PA_LD_LIN2 = 2, PA_LD_POOL = 3 };
// What the epilogue of a conv / elementwise backward kernel does with its value v:
//   PLAIN: store bf16(v)
//   STATS: store bf16(v) and accumulate per-channel sum / sum of squares of the stored value
//          (forward BatchNorm statistics fused into the producer)
//   BWD  : v is the gradient w.r.t. a = relu(s*x+t); store dz = v*[s*x+t>0] and accumulate
//          per-channel sum(dz), sum(dz*xhat), xhat=(x-mean)*invstd   (BatchNorm backward
//          reductions fused into the producer of the gradient)
enum { PA_OUT_PLAIN = 0, PA_OUT_STATS = 1, PA_OUT_BWD = 2 };
#define PA_FIN_SMALL_ROWS 128      // most partial rows a consumer finalizes in its prologue (bn_fin.h)
