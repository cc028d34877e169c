// VICReg loss for MI355X (gfx950): invariance MSE + variance hinge + off-diagonal covariance^2.  This file: the forward's
// column pass and final reduction, the workspace layout, the choice of side for the covariance term, and the C ABI.
//
// Replaces the reference's VICReg.loss (vicreg.py:35-58) and off_diagonal (:73-76):
//   repr = mse(x, y); x -= mean_b(x); std = sqrt(var_unbiased + 1e-4); std_loss = mean(relu(1 - std))/2 (+ y)
//   cov = x^T x / (cfg.vicreg.batch_size - 1)   <- the CONFIGURED batch size, not x.shape[0]
//   cov_loss = sum_{i != j} cov_ij^2 / embeddim (+ y);  loss = sim*repr + std*std_loss + cov*cov_loss
//
// Forward = three stages (vicreg_stage_ld):
//   0  vicreg_colstats_kernel<NR>  per 32 columns: column mean (fp32), centred sum of squares, sum (x-y)^2, hinge
//                                  partial, and the centred matrix cast to bf16 -- centring is done in fp32 BEFORE the
//                                  cast -- both TRANSPOSED, Xt[D][Kpad] (feature-major, batch contiguous, through an LDS
//                                  tile) and batch-major, Xc[Kpad][D].  NR by padded batch: 4 / 8 / 16 / 32 keep the rows
//                                  in registers up to Kpad = 128 / 256 / 512 / 1024, 0 re-reads them (any batch).
//   1  the one dense contraction   sum_{i != j} C_ij^2, C = Xc^T Xc, as fp64 partials: from the batch side, ||Xc Xc^T||_F^2
//                                  minus C's diagonal (vicreg_grad_kernels.hip: vicreg_launch_batch_gram), where the
//                                  padded batch is no larger than D and D is a multiple of 8 (vicreg_batch_side); else
//                                  from the feature side, the D x D Gram itself (vicreg_dxd_kernels.hip)
//   2  vicreg_finish_kernel        fixed-order reduction of all partials -> (loss, repr, std, cov)
// The backward (ias_vicreg_backward4_ld) is in vicreg_grad_kernels.hip; vicreg_tiles.h holds the tile products both
// sides share, vicreg_internal.h what crosses between the three files.
#include "vicreg_tiles.h"
#include "vicreg_internal.h"
#include <cstdlib>

#define VC_COLS 32        // columns per colstats workgroup: D / 32 = 256 workgroups at D = 8192, one per CU (64 columns
                          // per workgroup left half the chip idle: 60 us at B = 1024 against an HBM time of ~30)
#define VC_THREADS 1024  // 16 waves per workgroup: the column pass is latency-bound with few workgroups

// x, y: [B, D] fp32.  Xt_*: [D][Kpad] bf16 (zero padded in k).  colstats: [4][D] = mean_x, mean_y, m2_x, m2_y
// msepart: [gridDim.x] fp64.
// A wave covers the workgroup's 32 columns (128-byte row segments) of TWO rows at a time: lane = (row half, column).
// NR > 0: batch <= 32 NR, every thread keeps its NR rows of x and y in registers between the two passes (x and y are
// read ONCE); NR = 0: any batch, the second pass reads them again.
template <int NR>
__global__ __launch_bounds__(VC_THREADS) void vicreg_colstats_kernel(
    const float* __restrict__ x, const float* __restrict__ y, unsigned short* __restrict__ Xt_x,
    unsigned short* __restrict__ Xt_y, float* __restrict__ colstats, double* __restrict__ msepart,
    double* __restrict__ hingepart, double* __restrict__ diagpart, unsigned short* __restrict__ Xc_x,
    unsigned short* __restrict__ Xc_y, int B, int D, int Kpad,
    size_t ld /* row stride of x and y in floats (>= D: x, y may be column blocks of a wider matrix) */) {
  constexpr int NW = VC_THREADS / 64, RPI = 2 * NW;              // rows per iteration of the workgroup
  __shared__ float s_red[6][NW][64];
  __shared__ float s_mean[2][VC_COLS];
  __shared__ unsigned short s_tile[2][VC_COLS][64 + 2];
  __shared__ double s_mse[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & (VC_COLS - 1), rsub = lane >> 5;
  const int j0 = blockIdx.x * VC_COLS, j = j0 + col;
  const bool jok = j < D;

  // pass 1: column sums (wave w takes rows 2 w + rsub, + 32, ...), sum (x-y)^2
  float sx = 0.f, sy = 0.f, se = 0.f;
  float keepx[NR > 0 ? NR : 1], keepy[NR > 0 ? NR : 1];
  if (NR > 0) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int b = 2 * wave + rsub + RPI * i;
      keepx[i] = 0.f; keepy[i] = 0.f;
      if (jok && b < B) { keepx[i] = x[(size_t)b * ld + j]; keepy[i] = y[(size_t)b * ld + j]; }
    }
#pragma unroll
    for (int i = 0; i < NR; ++i) {                               // (rows beyond B hold zeros: they add nothing)
      sx += keepx[i]; sy += keepy[i];
      const float d = keepx[i] - keepy[i];
      se = fmaf(d, d, se);
    }
  } else {
    for (int b = 2 * wave + rsub; b < B; b += RPI) {
      if (jok) {
        const float xv = x[(size_t)b * ld + j], yv = y[(size_t)b * ld + j];
        sx += xv; sy += yv;
        const float d = xv - yv;
        se = fmaf(d, d, se);
      }
    }
  }
  s_red[0][wave][lane] = sx; s_red[1][wave][lane] = sy;
  // mse: reduce within the wave, then across waves
  for (int d = 32; d > 0; d >>= 1) se += __shfl_xor(se, d, 64);
  if (lane == 0) s_mse[wave] = (double)se;
  __syncthreads();
  if (wave == 0 && lane < VC_COLS) {
    float mx = 0.f, my = 0.f;
    for (int w = 0; w < NW; ++w) {                               // fixed order: waves, row halves
      mx += s_red[0][w][lane]; mx += s_red[0][w][lane + 32];
      my += s_red[1][w][lane]; my += s_red[1][w][lane + 32];
    }
    s_mean[0][lane] = mx / (float)B;
    s_mean[1][lane] = my / (float)B;
    if (lane == 0) {
      double m = 0.0;
      for (int w = 0; w < NW; ++w) m += s_mse[w];
      msepart[blockIdx.x] = m;
    }
  }
  __syncthreads();
  const float mx = s_mean[0][col], my = s_mean[1][col];

  // pass 2: centred sum of squares + bf16 transpose, 64 rows at a time
  float qx = 0.f, qy = 0.f, rx = 0.f, ry = 0.f;                 // (r*: the same sums over the bf16-ROUNDED values)
  auto chunk = [&](const int c64) {
    const int b0 = 64 * c64;
#pragma unroll
    for (int u = 0; u < 2; ++u) {                                // rows r = 2 wave + rsub (+ 32) of this 64-row chunk
      const int r = 2 * wave + rsub + RPI * u;
      const int b = b0 + r;
      float cx = 0.f, cy = 0.f;
      if (jok && b < B) {
        if (NR > 0) {
          cx = keepx[(2 * c64 + u) < NR ? 2 * c64 + u : 0] - mx;
          cy = keepy[(2 * c64 + u) < NR ? 2 * c64 + u : 0] - my;
        } else {
          cx = x[(size_t)b * ld + j] - mx;
          cy = y[(size_t)b * ld + j] - my;
        }
        qx = fmaf(cx, cx, qx);
        qy = fmaf(cy, cy, qy);
      }
      const unsigned short bx = f2bf(cx), by = f2bf(cy);
      const float fx = __uint_as_float((unsigned)bx << 16), fy = __uint_as_float((unsigned)by << 16);
      rx = fmaf(fx, fx, rx);
      ry = fmaf(fy, fy, ry);
      s_tile[0][col][r] = bx;
      s_tile[1][col][r] = by;
      // the same values batch-major, Xc[Kpad][D] (zero rows beyond B): the backward's B x B Gram contracts over D
      if (jok) { Xc_x[(size_t)b * D + j] = bx; Xc_y[(size_t)b * D + j] = by; }
    }
    __syncthreads();
    // write out: 32 columns x 64 k as 128-byte rows; thread -> (column c = tid/4, 16 k values)
    {
      const int c = tid >> 2, part = tid & 3;
      if (tid < 4 * VC_COLS && j0 + c < D) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          unsigned short* dst = (m == 0 ? Xt_x : Xt_y) + (size_t)(j0 + c) * Kpad + b0 + part * 16;
          unsigned int pk[8];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            pk[e] = (unsigned int)s_tile[m][c][part * 16 + 2 * e] | ((unsigned int)s_tile[m][c][part * 16 + 2 * e + 1] << 16);
          uint4* d4 = reinterpret_cast<uint4*>(dst);
          d4[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
          d4[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        }
      }
    }
    __syncthreads();
  };
  if constexpr (NR > 0) {
#pragma unroll
    for (int c64 = 0; c64 < (NR + 1) / 2; ++c64) {
      if (64 * c64 >= Kpad) break;
      chunk(c64);
    }
  } else {
    for (int c64 = 0; 64 * c64 < Kpad; ++c64) chunk(c64);
  }
  s_red[2][wave][lane] = qx; s_red[3][wave][lane] = qy;
  s_red[4][wave][lane] = rx; s_red[5][wave][lane] = ry;
  __syncthreads();
  const bool fin = wave == 0 && lane < VC_COLS && j0 + lane < D;
  float ax = 0.f, ay = 0.f, tx = 0.f, ty = 0.f;
  if (fin) {
    for (int w = 0; w < NW; ++w) {
      ax += s_red[2][w][lane]; ax += s_red[2][w][lane + 32];
      ay += s_red[3][w][lane]; ay += s_red[3][w][lane + 32];
      tx += s_red[4][w][lane]; tx += s_red[4][w][lane + 32];
      ty += s_red[5][w][lane]; ty += s_red[5][w][lane + 32];
    }
    colstats[0 * (size_t)D + j0 + lane] = s_mean[0][lane];
    colstats[1 * (size_t)D + j0 + lane] = s_mean[1][lane];
    colstats[2 * (size_t)D + j0 + lane] = ax;
    colstats[3 * (size_t)D + j0 + lane] = ay;
  }
  // variance hinge partial of this column block
  if (wave == 0) {
    float h = 0.f;
    if (fin) {
      const float inv_bm1 = 1.0f / (float)(B - 1);
      h = fmaxf(1.0f - sqrtf(ax * inv_bm1 + 0.0001f), 0.f) + fmaxf(1.0f - sqrtf(ay * inv_bm1 + 0.0001f), 0.f);
    }
    for (int d = 32; d > 0; d >>= 1) h += __shfl_xor(h, d, 64);
    if (lane == 0) hingepart[blockIdx.x] = (double)h;
    // the diagonal of the D x D Gram of the ROUNDED matrices, squared and summed: what the batch-side form of the
    // covariance term (vicreg_stage_ld) takes off ||Xc Xc^T||_F^2
    double dg = (double)tx * (double)tx + (double)ty * (double)ty;
    for (int d = 32; d > 0; d >>= 1) dg += __shfl_xor(dg, d, 64);
    if (lane == 0) diagpart[blockIdx.x] = dg;
  }
}

// out[0..3] = loss, repr_loss, std_loss, cov_loss (fp32): fixed-order reduction of every partial, by 256 threads.
// gram_x (+ gram_y): partial sums of squares; diagpart (batch-side form, else null): [nmse], taken off.
struct VcFinish {
  const double *hingepart, *msepart, *gram_x, *gram_y, *diagpart;
  int nmse, ngram, B, D, cfg_batch;
  float sim_coeff, std_coeff, cov_coeff;
  float* out;
};
// (A variant in which the fold's last-arriving workgroup did this reduction -- ticket counter, device-scope loads -- cost
// more than the launch it saved: +0 us at B = 128, +6 us at B = 1024, HISTORY.md round 4.)
__global__ __launch_bounds__(256) void vicreg_finish_kernel(const VcFinish f) {
  __shared__ double s[256][4];
  double mse = 0.0, hinge = 0.0, gx = 0.0, gy = 0.0;
  for (int i = threadIdx.x; i < f.nmse; i += 256) mse += f.msepart[i];
  for (int i = threadIdx.x; i < f.ngram; i += 256) { gx += f.gram_x[i]; if (f.gram_y) gy += f.gram_y[i]; }
  if (f.diagpart)                                                // gram_x holds sum G_ab^2 = sum over ALL of C: take C's diagonal off
    for (int i = threadIdx.x; i < f.nmse; i += 256) gy -= f.diagpart[i];
  for (int i = threadIdx.x; i < f.nmse; i += 256) hinge += f.hingepart[i];
  s[threadIdx.x][0] = mse; s[threadIdx.x][1] = hinge; s[threadIdx.x][2] = gx; s[threadIdx.x][3] = gy;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (threadIdx.x < d)
      for (int k = 0; k < 4; ++k) s[threadIdx.x][k] += s[threadIdx.x + d][k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double repr = s[0][0] / ((double)f.B * (double)f.D);
    const double stdl = s[0][1] / (2.0 * (double)f.D);
    const double den = (double)(f.cfg_batch - 1);
    const double cov = (s[0][2] + s[0][3]) / (den * den) / (double)f.D;
    f.out[0] = (float)((double)f.sim_coeff * repr + (double)f.std_coeff * stdl + (double)f.cov_coeff * cov);
    f.out[1] = (float)repr;
    f.out[2] = (float)stdl;
    f.out[3] = (float)cov;
  }
}
// ------------------------------------------------------------------------ C ABI
static inline size_t vc_align(size_t x) { return (x + 255) / 256 * 256; }
// IAS_VICREG_GRAM128=1 (diagnostics): the 128 x 128 register-staged kernels of round 2 for batch > 128 as well
static bool vicreg_force128() {
  static const bool v = ias_diag_env("IAS_VICREG_GRAM128") != nullptr && atoi(ias_diag_env("IAS_VICREG_GRAM128")) != 0;
  return v;
}
// The covariance term from the batch side.  sum_{i != j} C_ij^2 with C = Xc^T Xc (D x D) equals ||G||_F^2 - sum_j C_jj^2
// with G = Xc Xc^T (B x B): the same number from 2 B^2 D flops instead of 2 B D^2, and G is what the backward needs
// anyway (G vc).  Taken whenever the padded batch is no larger than the embedding (B = 128 / 1024 against D = 8192: 64x /
// 8x fewer flops); the feature-side kernels stay for batch > D.  No cancellation on this side of the switch: C has rank
// < B, so ||C||_F^2 >= (tr C)^2 / (B - 1) >= D / (B - 1) times its diagonal's share.
// Which side is taken is a pure function of the shape: the library keeps no state.  (Diagnostic library only:
// ias_vicreg_set_form(0 / 1 / -1) = feature side always / batch side where it applies / default, and the environment
// switch IAS_VICREG_DXD=1 -> 0: bench.py times the D x D kernels of rounds 1-3 through THAT library for `roofline.dxd`.)
#ifdef IAS_DIAG
static int g_vicreg_form = -1;
extern "C" int ias_vicreg_set_form(int form) {
  if (form < -1 || form > 1) return IAS_ERR_ARG;
  g_vicreg_form = form;
  return IAS_OK;
}
static bool vicreg_feature_side_forced() {
  static const bool env_dxd = ias_diag_env("IAS_VICREG_DXD") != nullptr && atoi(ias_diag_env("IAS_VICREG_DXD")) != 0;
  return g_vicreg_form < 0 ? env_dxd : g_vicreg_form == 0;
}
#else
static constexpr bool vicreg_feature_side_forced() { return false; }
#endif
static bool vicreg_batch_side(int Kpad, int D) { return !vicreg_feature_side_forced() && D >= 8 && (D & 7) == 0 && Kpad <= D; }

VicregWs vicreg_ws(int B, int D) {
  VicregWs w;
  w.Kpad = (B + GT - 1) / GT * GT;   // multiple of 128: the pair kernel's depth, the backward's batch tiles (zero padded)
  w.ntile = (D + GT - 1) / GT;
  w.ngram = w.ntile * (w.ntile + 1) / 2;
  w.nmse = (D + VC_COLS - 1) / VC_COLS;
  size_t o = 0;
  w.xt_x = o;     o = vc_align(o + sizeof(unsigned short) * (size_t)D * w.Kpad);
  w.xt_y = o;     o = vc_align(o + sizeof(unsigned short) * (size_t)D * w.Kpad);
  w.colstats = o; o = vc_align(o + sizeof(float) * 4 * (size_t)D);
  w.mse = o;      o = vc_align(o + sizeof(double) * w.nmse);
  w.hinge = o;    o = vc_align(o + sizeof(double) * w.nmse);
  w.diag = o;     o = vc_align(o + sizeof(double) * w.nmse);
  w.gram_x = o;   o = vc_align(o + sizeof(double) * w.ngram);
  w.gram_y = o;   o = vc_align(o + sizeof(double) * w.ngram);
  // backward: centred bf16 copies batch-major [Kpad][D], and the two B x B Grams [2][Kpad][Kpad] fp32
  w.xc_x = o;     o = vc_align(o + sizeof(unsigned short) * (size_t)D * w.Kpad);
  w.xc_y = o;     o = vc_align(o + sizeof(unsigned short) * (size_t)D * w.Kpad);
  // the B x B Gram is contracted over D in `nsplit` slices (enough workgroups for the chip at any batch size), each
  // slice writing its own partial Gram [nsplit][2][Kpad][Kpad]; vicreg_gconv_kernel adds them in slice order
  // batch > 128: the 256 x 256 LDS-DMA kernels (forward Gram; backward when D is a multiple of the 64-deep K-tile)
  w.t256 = w.Kpad > 128 && !vicreg_force128() && D >= 256 && (unsigned long long)D * (unsigned long long)w.Kpad < (1ull << 31);
  w.dual = vicreg_batch_side(w.Kpad, D);
  {
    const bool b256 = w.t256 && D % 64 == 0;
    w.b256 = b256;
    const int bt = b256 ? (w.Kpad + 255) / 256 : w.Kpad / GT, npair = bt * (bt + 1) / 2;
    int nsplit = (b256 ? 256 : 512) / (2 * npair);      // one resident round: 1 (256 tiles) / 2 (128 tiles) workgroups per CU
    if (nsplit < 1) nsplit = 1;
    if (nsplit > D / 256) nsplit = D / 256 > 0 ? D / 256 : 1;
    w.ksplit = ((D + nsplit - 1) / nsplit + GK - 1) / GK * GK;
    w.nsplit = (D + w.ksplit - 1) / w.ksplit;
  }
  w.bgram = o;    o = vc_align(o + sizeof(float) * 2 * (size_t)w.Kpad * w.Kpad * w.nsplit);
  w.bgram16 = o;  o = vc_align(o + sizeof(unsigned short) * 2 * (size_t)w.Kpad * w.Kpad);
  w.gdiag = o;    o = vc_align(o + sizeof(float) * 2 * (size_t)w.Kpad);
  {                                                              // partial sums of G_ab^2, one or two per fold workgroup
    const int bt2 = (w.Kpad + 255) / 256;
    size_t cgrid = (2 * (size_t)w.Kpad * w.Kpad + 255) / 256;
    if (cgrid > 2048) cgrid = 2048;
    w.ng2 = w.b256 ? 2 * 16 * (bt2 * (bt2 + 1) / 2) : 2 * (int)cgrid;
  }
  w.g2part = o;   o = vc_align(o + sizeof(double) * (size_t)w.ng2);
  w.total = o;
  return w;
}

extern "C" long long ias_vicreg_workspace_bytes(int B, int D) {
  if (B < 2 || D < 1) return IAS_ERR_ARG;
  return (long long)vicreg_ws(B, D).total;
}

// x, y [B,D] fp32 -> out[4] = (loss, repr_loss, std_loss, cov_loss).  cfg_batch = the configured batch
// size whose (cfg_batch - 1) divides the covariance (vicreg.py:47-48).  After the call the workspace
// holds colstats [4][D] (mean_x, mean_y, centred sum of squares x / y) at VicregWs::colstats.
// stage < 0: the whole loss; 0: column pass (means, centred bf16 transposes, MSE / hinge partials); 1: the Gram
// kernel(s) on the matrix cores; 2: the final reduction.  Stages run on a workspace the earlier stages have filled
// (bench.py times stage 1 alone with HIP events for the MFMA roofline).
static int vicreg_stage_ld(int stage, const float* x, const float* y, long long ld, float* out, void* workspace,
                           long long workspace_bytes, int B, int D, int cfg_batch, float sim_coeff, float std_coeff,
                           float cov_coeff, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !y || !out || !workspace || B < 2 || D < 1 || cfg_batch < 2 || stage > 2 || ld < D) return IAS_ERR_ARG;
  const VicregWs w = vicreg_ws(B, D);
  if ((size_t)workspace_bytes < w.total) return IAS_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  unsigned short* xt_x = (unsigned short*)(ws + w.xt_x);
  unsigned short* xt_y = (unsigned short*)(ws + w.xt_y);
  float* colstats = (float*)(ws + w.colstats);
  double* mse = (double*)(ws + w.mse);
  double* hinge = (double*)(ws + w.hinge);
  if (stage < 0 || stage == 0)
  {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(w.nmse), dim3(VC_THREADS), 0, stream, x, y, xt_x, xt_y, colstats, mse, hinge,
                         (double*)(ws + w.diag), (unsigned short*)(ws + w.xc_x), (unsigned short*)(ws + w.xc_y), B, D, w.Kpad,
                         (size_t)ld);
    };
    static const bool reread = ias_diag_env("IAS_VICREG_COLSTATS_REREAD") != nullptr;   // (diagnostics: the two-read form at any batch)
    if (reread || w.Kpad > 1024) launch(vicreg_colstats_kernel<0>);
    else if (w.Kpad <= 128) launch(vicreg_colstats_kernel<4>);
    else if (w.Kpad <= 256) launch(vicreg_colstats_kernel<8>);
    else if (w.Kpad <= 512) launch(vicreg_colstats_kernel<16>);
    else launch(vicreg_colstats_kernel<32>);
  }
  VcFinish fin;
  fin.hingepart = hinge; fin.msepart = mse; fin.nmse = w.nmse;
  fin.B = B; fin.D = D; fin.cfg_batch = cfg_batch;
  fin.sim_coeff = sim_coeff; fin.std_coeff = std_coeff; fin.cov_coeff = cov_coeff;
  fin.out = out;
  if (w.dual) {
    // batch side: G = Xc Xc^T in D-slices, folded (and squared, summed) in slice order; the backward finds G in place
    if (w.Kpad % GT) return IAS_ERR_UNSUPPORTED;
    fin.gram_x = (const double*)(ws + w.g2part); fin.gram_y = nullptr; fin.ngram = w.ng2;
    fin.diagpart = (const double*)(ws + w.diag);
    if (stage < 0 || stage == 1) vicreg_launch_batch_gram(w, ws, D, stream, true);
    if (stage < 0 || stage == 2) hipLaunchKernelGGL(vicreg_finish_kernel, dim3(1), dim3(256), 0, stream, fin);
    return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
  }
  // feature side: the D x D Gram's off-diagonal square sums, per tile or run of tiles
  fin.gram_x = (const double*)(ws + w.gram_x); fin.gram_y = (const double*)(ws + w.gram_y); fin.diagpart = nullptr;
  fin.ngram = vicreg_launch_feature_gram(w, ws, D, stream, stage < 0 || stage == 1);
  if (stage < 0 || stage == 2) hipLaunchKernelGGL(vicreg_finish_kernel, dim3(1), dim3(256), 0, stream, fin);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_vicreg_stage(int stage, const float* x, const float* y, float* out, void* workspace,
                                long long workspace_bytes, int B, int D, int cfg_batch, float sim_coeff, float std_coeff,
                                float cov_coeff, void* stream_) {
  return vicreg_stage_ld(stage, x, y, D, out, workspace, workspace_bytes, B, D, cfg_batch, sim_coeff, std_coeff, cov_coeff,
                         stream_);
}

extern "C" int ias_vicreg_loss(const float* x, const float* y, float* out, void* workspace, long long workspace_bytes,
                               int B, int D, int cfg_batch, float sim_coeff, float std_coeff, float cov_coeff,
                               void* stream_) {
  return vicreg_stage_ld(-1, x, y, D, out, workspace, workspace_bytes, B, D, cfg_batch, sim_coeff, std_coeff, cov_coeff,
                         stream_);
}

// The same loss on x, y that are column blocks of wider row-major matrices (row stride ld >= D floats): the gathered
// [W B_l, 2 D] buffer of FullGatherLayer(cat(x, y, dim=1)) is consumed in place, x = buf[:, :D], y = buf[:, D:].
extern "C" int ias_vicreg_loss_ld(const float* x, const float* y, long long ld, float* out, void* workspace,
                                  long long workspace_bytes, int B, int D, int cfg_batch, float sim_coeff, float std_coeff,
                                  float cov_coeff, void* stream_) {
  return vicreg_stage_ld(-1, x, y, ld, out, workspace, workspace_bytes, B, D, cfg_batch, sim_coeff, std_coeff, cov_coeff,
                         stream_);
}

// The backward (vicreg_grad_kernels.hip) with the four cotangents as separate device floats, any of them null (= zero):
// what autograd hands over when only some of the four outputs were differentiated -- no packing kernel in front.  x, y
// with row stride ld, gx, gy WRITTEN with row stride ldg (the two column blocks of the [W B_l, 2 D] cotangent that
// FullGatherLayer's backward reduce-scatters: no split / cat copies either way).
extern "C" int ias_vicreg_backward4_ld(const float* x, const float* y, long long ld, const float* g_loss, const float* g_repr,
                                       const float* g_std, const float* g_cov, float* gx, float* gy, long long ldg,
                                       void* workspace, long long workspace_bytes, int B, int D, int cfg_batch,
                                       float sim_coeff, float std_coeff, float cov_coeff, void* stream_) {
  return vicreg_backward_ld(x, y, ld, VcCot{{g_loss, g_repr, g_std, g_cov}}, gx, gy, ldg, workspace, workspace_bytes, B, D,
                            cfg_batch, sim_coeff, std_coeff, cov_coeff, stream_);
}
