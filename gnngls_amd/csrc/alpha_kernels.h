// alpha_kernels.h -- internal interface between the alpha-nearness kernel (alpha_kernels.hip) and the C ABI (capi.hip).
//
// alpha(e) = (cost of the minimum 1-tree forced through e) - (cost of the minimum 1-tree) under Held-Karp potentials pi
// (Helsgaun's alpha-nearness): the classical relaxation of the regret the model predicts, exact and model-free.  The definition
// -- canonical weight, beta as the minimax-path value, node 0's rule -- is the contract stated in include/gnngls_hip.h; every
// value is selected by comparisons or is one subtraction, so the matrix is bit-determined by (D, pi).  One workgroup per
// instance, one launch per batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

// a node's Prim key, parent and potential live in registers (at most four nodes per lane, at most four wavefronts per instance);
// node and parent share a 20-bit selection key
constexpr int kAlphaMaxN = 1024;
constexpr int kAlphaStatusAsymmetric = 3;      // GNNGLS_STATUS_ASYMMETRIC

// D [B,n,n], pi [B,n] or NULL (all zeros); alpha [B,n,n], status [B].  3 <= n <= kAlphaMaxN, B >= 1.
hipError_t launch_alpha_nearness(const double *D, const double *pi, int B, int n, double *alpha, int32_t *status, hipStream_t stream);

// workgroup size of the launch for n nodes (64: one wavefront, n <= 256) and its dynamic LDS
int alpha_threads(int n);
int alpha_lds_bytes(int n);

}  // namespace gnngls
