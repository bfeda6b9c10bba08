// Backward of the bilinear warp (warp_kernel of pose_ops.hip): launch interface and the chain rule from d loss / d tinv to the
// augmentation parameters, shared by the device finish kernel (warp_bwd.hip) and the host entry pa_affine_params_bwd_host (api.hip).
#pragma once
#include "common.h"
#include <math.h>

#define PA_WARP_BWD_ROWS 8          // output rows per workgroup of launch 1 (a strip); the last strip of a sample may be shorter

// strips per sample; 0 for a shape the launch does not take (B < 1, res < 1, or more than 2^31 - 1 workgroups)
inline long pa_warp_bwd_strips(int B, int res) {
    if (B < 1 || res < 1) return 0;
    const long n = ((long)res + PA_WARP_BWD_ROWS - 1) / PA_WARP_BWD_ROWS;
    return n * (long)B > 0x7fffffffL ? 0 : n;
}
inline size_t pa_warp_bwd_workspace_size(int B, int res) { return (size_t)pa_warp_bwd_strips(B, res) * (size_t)(B > 0 ? B : 0) * 9 * sizeof(double); }

// pa_affine_params builds tinv = invert_affine(make_transform(cx, cy, s, rot, res, 200)); with k = 200 s / res, th = -rot pi / 180, hr = res / 2:
//   tinv = [ k cos th,  k sin th,  cx - k hr (cos th + sin th);
//           -k sin th,  k cos th,  cy - k hr (cos th - sin th) ]
// (make_transform's rot == 0 branch is this at th = 0).  p = {cx, cy, s, rot, flip, gain r g b}, G = d loss / d tinv [6], dgain [3] or
// nullptr (zeros) -> out[8] = d loss / d {cx, cy, s, rot per degree, flip (always 0), gain r g b}.
__host__ __device__ inline void pa_affine_params_chain(const double* p, const double* G, const double* dgain, double res, double* out) {
    const double k = 200.0 * p[2] / res, hr = res / 2;
    const double th = -p[3] * 3.14159265358979323846 / 180.0;
    const double sn = sin(th), cs = cos(th);
    const double dk = G[0] * cs + G[1] * sn - G[2] * hr * (cs + sn) - G[3] * sn + G[4] * cs - G[5] * hr * (cs - sn);
    const double dth = k * (-G[0] * sn + G[1] * cs - G[2] * hr * (cs - sn) - G[3] * cs - G[4] * sn + G[5] * hr * (cs + sn));
    out[0] = G[2];
    out[1] = G[5];
    out[2] = dk * (200.0 / res);
    out[3] = dth * (-3.14159265358979323846 / 180.0);
    out[4] = 0.0;
    out[5] = dgain ? dgain[0] : 0.0;
    out[6] = dgain ? dgain[1] : 0.0;
    out[7] = dgain ? dgain[2] : 0.0;
}

// dimg: fp32, layout 0 [B][3][res][res] or 1 [B][res][res][4] (16-byte aligned); workspace: pa_warp_bwd_workspace_size bytes, 8-byte aligned;
// dtinv [B][6], dgain [B][3], dparams [B][8]: each optional
int pa_launch_warp_bwd(const unsigned char* src, int Hs, int Ws, const int* sizes, const double* tinv, const double* params, int B, int res,
                       const float* dimg, int layout, void* workspace, double* dtinv, double* dgain, double* dparams, hipStream_t st);
