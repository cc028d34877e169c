// Private to the three VICReg kernel files: the workspace layout and the plain C++ host functions that cross between
// them.  None is an entry point of the C ABI (include/ias_hip.h): hidden visibility, the libraries export none of them.
#pragma once
#include "ias_common.h"

#define VC_HIDDEN __attribute__((visibility("hidden")))

// Byte offsets into the caller's workspace, the derived sizes, and which kernels the shape takes (vicreg_ws,
// vicreg_kernels.hip).
struct VicregWs { size_t xt_x, xt_y, colstats, mse, hinge, diag, gram_x, gram_y, xc_x, xc_y, bgram, bgram16, gdiag, g2part, total; int Kpad, ntile, ngram, nmse, nsplit, ksplit, ng2; bool t256, b256, dual; };
VC_HIDDEN VicregWs vicreg_ws(int B, int D);

// The cotangents of (loss, repr_loss, std_loss, cov_loss): one device float each, null = zero (autograd hands the unused
// outputs over as None; packing them into one buffer cost a concatenation kernel per backward).
struct VcCot { const float* g[4]; };

// vicreg_dxd_kernels.hip.  The feature-side Gram C = Xt Xt^T of both branches, squared and summed without its diagonal
// into fp64 partials at w.gram_x / w.gram_y; returns how many partials per branch the finish kernel has to add.
// launch = false: only that count (the finish stage run on its own).
VC_HIDDEN int vicreg_launch_feature_gram(const VicregWs& w, char* ws, int D, hipStream_t stream, bool launch);

// vicreg_grad_kernels.hip.  G = Xc Xc^T for both branches: partial Grams per D-slice [nsplit][2][Kpad][Kpad] (every word
// written), folded in slice order to bf16 (diagonal apart, fp32); `squares` (forward): the fold also leaves the partial
// sums of G_ab^2 at w.g2part.
VC_HIDDEN void vicreg_launch_batch_gram(const VicregWs& w, char* ws, int D, hipStream_t stream, bool squares);
// Backward of ias_vicreg_loss on the SAME workspace (it must still hold the forward's column statistics and centred
// bf16 copies -- and, after a batch-side forward, G): the cotangents gcoef -> gx, gy [B,D] fp32, written with row stride ldg.
VC_HIDDEN int vicreg_backward_ld(const float* x, const float* y, long long ld, const VcCot gcoef, float* gx, float* gy,
                                 long long ldg, void* workspace, long long workspace_bytes, int B, int D, int cfg_batch,
                                 float sim_coeff, float std_coeff, float cov_coeff, void* stream_);
