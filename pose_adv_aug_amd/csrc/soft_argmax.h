// Soft-arg-max over heat maps and its backward pass (soft_argmax.hip): launch interface.
#pragma once
#include "common.h"

#define PA_SAM_THREADS 1024         // workgroup of the joint-minor forward kernel: one per (sample, group of four joints)
#define PA_SAM_INFLIGHT 4           // 16-byte loads of a thread in flight per trip: a trip covers PA_SAM_INFLIGHT * PA_SAM_THREADS pixels
#define PA_SAM_GENERIC_THREADS 256  // workgroup of the strided kernels: one per (sample, joint) map
#define PA_SAM_BWD_THREADS 256      // workgroup of the joint-minor backward kernel
#define PA_SAM_BWD_CHUNKS 4         // 16-byte chunks per thread the joint-minor backward grid is sized for

// maps / dmaps: fp32, layout 0 [B][J][H][W] or 1 [B][H*W][J]; coords [B][J][2] fp32; state [B][J][4] double = m, Z, ex, ey; dcoords [B][J][2] fp32.
// The arguments are checked once, in pa_soft_argmax / pa_soft_argmax_bwd (api.hip): H * W < 2^27 and B * J < 2^31.
int pa_launch_soft_argmax(const float* maps, int layout, int B, int J, int H, int W, float beta, float* coords, double* state, hipStream_t st);
int pa_launch_soft_argmax_bwd(const float* maps, int layout, int B, int J, int H, int W, float beta, const double* state, const float* dcoords,
                              float* dmaps, hipStream_t st);
// y[i] = the device's double exp(x[i]), the function the kernels above call (calibration of the test bound)
int pa_launch_exp_probe(const double* x, double* y, size_t n, hipStream_t st);
