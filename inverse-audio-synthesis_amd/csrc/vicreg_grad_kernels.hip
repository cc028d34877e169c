// VICReg from the batch side: the B x B Gram G = Xc Xc^T and the backward.
//
// d loss / d x, d loss / d y of the reference's VICReg.loss (vicreg.py:35-58) in closed form, never forming a D x D
// matrix.  With vc = v - mean_b(v) (v = x or y), m2_j = sum_b vc_bj^2, s_j = sqrt(m2_j / (B - 1) + 1e-4), G = vc vc^T
// (B x B), and the incoming cotangents folded into a = g_loss sim + g_repr, b = g_loss std + g_std, c = g_loss cov + g_cov:
//   grad_v = +-a 2 (x - y) / (B D)  -  b [s_j < 1] vc / (2 D (B - 1) s_j)  +  c kappa (G vc - vc m2_j),
//   kappa = 4 / ((cfg_batch - 1)^2 D)          (the centring adjoint vanishes: every column of the sum is zero-mean)
// G is also what the forward's covariance term is taken from where the padded batch is no larger than D
// (vicreg_batch_side, vicreg_kernels.hip); the backward then finds it in the workspace.  Xc [Kpad][D] and Xt [D][Kpad]
// are the centred bf16 copies the column pass leaves.  Which kernels by shape (VicregWs::b256 = Kpad > 128, D >= 256,
// D % 64 == 0, D Kpad < 2^31, no IAS_VICREG_GRAM128):
//   G, one D-slice per workgroup   vicreg_bgram256_kernel (b256: 256 x 256 tiles, g2_product), else vicreg_bgram_kernel
//                                  (128 x 128 tiles, vc_tile_product); each slice writes its own partial Gram
//   fold of the slices             vicreg_gconv256_kernel (b256), else vicreg_gconv_kernel: summed in slice order
//                                  (deterministic), cast to bf16 with the diagonal apart in fp32, G_ab^2 summed
//   (G - diag) vc + the rest       vicreg_grad256_kernel (b256); vicreg_grad128_kernel (Kpad == 128 and 16-byte aligned
//                                  x, y, gx, gy: both branches per workgroup); else vicreg_grad_kernel
#include "vicreg_tiles.h"
#include "vicreg_internal.h"

__device__ __forceinline__ void vc_cot_coefs(const VcCot& k, float sim_coeff, float std_coeff, float cov_coeff, float& ca,
                                             float& cb, float& cc) {
  const float gl = k.g[0] ? *k.g[0] : 0.0f;
  ca = gl * sim_coeff + (k.g[1] ? *k.g[1] : 0.0f);
  cb = gl * std_coeff + (k.g[2] ? *k.g[2] : 0.0f);
  cc = gl * cov_coeff + (k.g[3] ? *k.g[3] : 0.0f);
}

// What the gradient epilogue needs that is the same for every element:
//   grad_v[b][j] = +-repr_k (x - y) + av_j vc + cck ((G - diag) vc + G_bb vc),   + for x, - for y
struct VcGradK { float repr_k, cb, cck, inv_bm1; };
__device__ __forceinline__ VcGradK vc_grad_k(const VcCot& gcoef, float sim_coeff, float std_coeff, float cov_coeff, int B,
                                             int D, int cfg_batch) {
  float ca, cb, cc;
  vc_cot_coefs(gcoef, sim_coeff, std_coeff, cov_coeff, ca, cb, cc);
  const float kappa = 4.0f / ((float)(cfg_batch - 1) * (float)(cfg_batch - 1) * (float)D);
  return {ca * 2.0f / ((float)B * (float)D), cb, cc * kappa, 1.0f / (float)(B - 1)};
}
// av of a column with centred sum of squares m2, the coefficient of vc: variance hinge (active where s < 1) and the
// diagonal part of the covariance term
__device__ __forceinline__ float vc_col_av(const VcGradK& k, float m2, int B, int D) {
  const float sd = sqrtf(m2 * k.inv_bm1 + 0.0001f);
  return (sd < 1.0f ? -k.cb / (2.0f * (float)D * (float)(B - 1) * sd) : 0.0f) - k.cck * m2;
}

// v += the nsplit partials of element i of the Gram (n elements apart), eight slices in flight, added in slice order.
// A macro: as a function, which the compiler optimises on its own before it inlines it, the same loop comes out with its
// blocks laid out differently, one more taken branch per group of eight (vicreg_gconv256_kernel at B = 1024, 12 slices:
// 18.9 -> 19.3 us).
#define VC_FOLD_SLICES(v, Gp, n, i, nsplit)                                                                          \
  for (int s0 = 0; s0 < (nsplit); s0 += 8) {                                                                         \
    float a[8];                                                                                                      \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) a[u] = s0 + u < (nsplit) ? (Gp)[(size_t)(s0 + u) * (n) + (i)] : 0.0f; \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) v += a[u];                                                         \
  }

// A 256 x 256 accumulator tile of g2_product leaves through LDS half by half (128 rows x 256 fp32 = 128 KB, the idle
// staging area: every wave has passed the product's last barrier), so that afterwards every thread owns 4 fixed columns
// and walks the rows with 16-byte accesses (1 KB per wave and row) instead of 64-byte fragments of four rows each.
// The 16-column groups are XOR-swizzled by the lane's row quarter: the accumulator stores are conflict-free.
// g2_stage_store: the accumulators of a wave of that half (wr == half) -> s_c; g2_stage_read: the thread's columns
// 4 (tid & 63) .. + 3 of row rl of the half.  A __syncthreads() between the two, and one before the next half's store.
// (Both take the lane's coordinates from threadIdx themselves: with them as parameters the compiler simplifies the
// index arithmetic without their ranges and the kernels come out with 18 more VGPRs.)
__device__ __forceinline__ void g2_stage_store(float* s_c, const vc_f32x4 (&acc)[8][4]) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wc = wave & 3, r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        s_c[(16 * m + 4 * q + e) * 256 + ((wc * 64 + 16 * n + r) ^ (q << 4))] = acc[m][n][e];
}
__device__ __forceinline__ vc_f32x4 g2_stage_read(const float* s_c, int rl) {
  const int c4 = threadIdx.x & 63;
  return *reinterpret_cast<const vc_f32x4*>(s_c + rl * 256 + ((4 * c4) ^ (((rl >> 2) & 3) << 4)));
}

// One upper-triangular 128 x 128 tile of one D-slice of G = Xc Xc^T per workgroup (grid: tiles x slices x branches).
// The slice's partial tile (and its mirror image) is WRITTEN to that slice's own Gram, once: no atomics, nothing to
// zero, and the sum over slices is taken in slice order by vicreg_gconv_kernel -- the backward is bit-reproducible
// (the reference trains with deterministic=True, pretrain.py:100).
__global__ __launch_bounds__(256, 2) void vicreg_bgram_kernel(const unsigned short* __restrict__ Xc_x,
                                                              const unsigned short* __restrict__ Xc_y, float* __restrict__ Gp,
                                                              int D, int Kpad, int ntile, int ksplit /* features per slice */) {
  __shared__ __attribute__((aligned(16))) unsigned short s_a[2][GT][GLD];
  __shared__ __attribute__((aligned(16))) unsigned short s_b[2][GT][GLD];
  int ti, tj;
  vc_tri_tile(blockIdx.x, ntile, ti, tj);
  const int branch = blockIdx.z;
  const unsigned short* Xc = branch ? Xc_y : Xc_x;
  float* Gb = Gp + ((size_t)blockIdx.y * 2 + branch) * Kpad * Kpad;
  const int kbeg = blockIdx.y * ksplit, kend = min(kbeg + ksplit, D);   // D % 8 == 0 is checked on the host
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  const int row0 = ti * GT, col0 = tj * GT;
  f32x16 acc[2][2];
  vc_zero(acc);
  vc_tile_product(Xc, (size_t)D, Kpad, Xc, (size_t)D, Kpad, row0, col0, kbeg, kend, s_a, s_b, acc);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = vc_c32_row(row0 + wr * 64 + m * 32, e, h);
        const int col = col0 + wc * 64 + n * 32 + r;
        Gb[(size_t)row * Kpad + col] = acc[m][n][e];
        if (ti != tj) Gb[(size_t)col * Kpad + row] = acc[m][n][e];
      }
}

// G = sum over the D-slices of their partial Grams, in slice order (fp32, both branches) -> bf16 with the diagonal taken
// out (it stays in fp32: gdiag[branch][b] = G_bb).  The diagonal of G is 10-100x its off-diagonal entries and would
// carry its bf16 rounding (2^-9) straight into the dominant term G_bb vc_bj of the gradient; the epilogue of
// vicreg_grad_kernel adds that term in fp32 instead.
__global__ __launch_bounds__(256) void vicreg_gconv_kernel(const float* __restrict__ Gp, unsigned short* __restrict__ Gb,
                                                           float* __restrict__ gdiag, int Kpad, int nsplit,
                                                           double* __restrict__ g2part /* [gridDim.x][2] or null */) {
  __shared__ double s_sq[4][2];
  const size_t n = (size_t)2 * Kpad * Kpad;
  double sq[2] = {0.0, 0.0};                                      // sum of G_ab^2 per branch (the diagonal included)
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t q = i / ((size_t)Kpad * Kpad), rem = i - q * (size_t)Kpad * Kpad;
    const int row = (int)(rem / Kpad), col = (int)(rem - (size_t)row * Kpad);
    float v = 0.0f;
    VC_FOLD_SLICES(v, Gp, n, i, nsplit);
    sq[q] += (double)v * (double)v;
    if (row == col) gdiag[q * Kpad + row] = v;
    Gb[i] = f2bf(row == col ? 0.0f : v);
  }
  if (g2part) {                                                  // fixed order: lanes (butterfly), then waves
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      for (int d = 32; d > 0; d >>= 1) sq[k] += __shfl_xor(sq[k], d, 64);
      if ((threadIdx.x & 63) == 0) s_sq[threadIdx.x >> 6][k] = sq[k];
    }
    __syncthreads();
    if (threadIdx.x < 2)
      g2part[2 * (size_t)blockIdx.x + threadIdx.x] =
          ((s_sq[0][threadIdx.x] + s_sq[1][threadIdx.x]) + s_sq[2][threadIdx.x]) + s_sq[3][threadIdx.x];
  }
}

// One 128 (batch rows) x 128 (features) tile of gx (branch 0) or gy (branch 1) per workgroup: the product (G - diag) vc
// through the double-buffered LDS panels, then the elementwise terms.  (Both branches in one workgroup, round 2, were 64
// workgroups at B = 128, D = 8192: a quarter of the chip.)
__global__ __launch_bounds__(256, 2) void vicreg_grad_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const unsigned short* __restrict__ Xt_x,
    const unsigned short* __restrict__ Xt_y, const unsigned short* __restrict__ Gb, const float* __restrict__ gdiag,
    const float* __restrict__ colstats,
    const VcCot gcoef /* g_loss, g_repr, g_std, g_cov */, float* __restrict__ gx, float* __restrict__ gy,
    int B, int D, int Kpad, int cfg_batch, float sim_coeff, float std_coeff, float cov_coeff, size_t ld, size_t ldg) {
  __shared__ __attribute__((aligned(16))) unsigned short s_a[2][GT][GLD];   // G rows (bf16)
  __shared__ __attribute__((aligned(16))) unsigned short s_b[2][GT][GLD];   // Xt rows (features)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const int col0 = blockIdx.x * GT, row0 = blockIdx.y * GT, branch = blockIdx.z;   // one branch per workgroup (grid.z = 2)
  const VcGradK k = vc_grad_k(gcoef, sim_coeff, std_coeff, cov_coeff, B, D, cfg_batch);

  f32x16 acc[2][2];   // [m][n]
  vc_zero(acc);
  vc_tile_product(Gb + (size_t)branch * Kpad * Kpad, (size_t)Kpad, Kpad, branch ? Xt_y : Xt_x, (size_t)Kpad, D, row0, col0, 0,
                  Kpad, s_a, s_b, acc);

  // epilogue: elementwise terms
  const float repr_k = branch ? -k.repr_k : k.repr_k;
  float* gout = branch ? gy : gx;
  const float* own = branch ? y : x;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int j = col0 + wc * 64 + n * 32 + r;
    if (j >= D) continue;
    const float mu = colstats[(size_t)branch * D + j], av = vc_col_av(k, colstats[(size_t)(2 + branch) * D + j], B, D);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int b = vc_c32_row(row0 + wr * 64 + m * 32, e, h);
        if (b >= B) continue;
        const size_t idx = (size_t)b * ld + j;
        const float xv = x[idx], yv = y[idx];
        const float v = own[idx] - mu;
        gout[(size_t)b * ldg + j] = repr_k * (xv - yv) + av * v + k.cck * (acc[m][n][e] + gdiag[(size_t)branch * Kpad + b] * v);
      }
  }
}

// ---- batch <= 128 (BASELINE configs[2]): both branches of a 128 (batch) x 64 (features) tile in one workgroup ---------
// The whole contraction (K = 128) fits in LDS at once: G_x, G_y (2 x 32 KB bf16) and the two 64 x 128 slabs of Xt are
// loaded with 16-byte accesses, one barrier, 16 MFMAs per wave (8 waves: 4 row blocks x 2 column blocks, both branches),
// then the two accumulator tiles go through LDS so that the elementwise epilogue reads x and y ONCE for both branches
// and moves 16 bytes per access (256-byte row segments).  vicreg_grad_kernel (one branch per workgroup, 4-byte accesses
// to x, y read twice) took 27 us at B = 128, D = 8192; it stays as the fallback for unaligned views.
#define G1_COLS 64
#define G1_LDK 136        // bf16 row stride of the staged operands (272 B)
#define G1_LDC 72         // fp32 row stride of the staged result (4 rows apart = 32 banks apart: the two lane halves)
#define G1_LDS_BYTES ((2 * 128 + 2 * G1_COLS) * G1_LDK * 2)
static_assert(2 * 128 * G1_LDC * 4 <= G1_LDS_BYTES, "the result tiles overlay the operands");
__global__ __launch_bounds__(512) void vicreg_grad128_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const unsigned short* __restrict__ Xt_x,
    const unsigned short* __restrict__ Xt_y, const unsigned short* __restrict__ Gb, const float* __restrict__ gdiag,
    const float* __restrict__ colstats, const VcCot gcoef, float* __restrict__ gx, float* __restrict__ gy,
    int B, int D, int cfg_batch, float sim_coeff, float std_coeff, float cov_coeff, size_t ld, size_t ldg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_g1[];
  unsigned short (*s_a)[128][G1_LDK] = reinterpret_cast<unsigned short (*)[128][G1_LDK]>(s_g1);
  unsigned short (*s_b)[G1_COLS][G1_LDK] =
      reinterpret_cast<unsigned short (*)[G1_COLS][G1_LDK]>(s_g1 + 2 * 128 * G1_LDK * 2);
  float (*s_c)[128][G1_LDC] = reinterpret_cast<float (*)[128][G1_LDC]>(s_g1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * G1_COLS;
  // ---- operands -> LDS (rows of 128 bf16 = 16 chunks of 16 bytes)
  {
    const int ch = tid & 15, r0 = tid >> 4;                      // 32 rows per pass
#pragma unroll
    for (int br = 0; br < 2; ++br) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + 32 * i;
        *reinterpret_cast<uint4*>(&s_a[br][row][ch * 8]) =
            *reinterpret_cast<const uint4*>(Gb + ((size_t)br * 128 + row) * 128 + ch * 8);
      }
      const unsigned short* Xt = br ? Xt_y : Xt_x;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = r0 + 32 * i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (j0 + row < D) v = *reinterpret_cast<const uint4*>(Xt + (size_t)(j0 + row) * 128 + ch * 8);
        *reinterpret_cast<uint4*>(&s_b[br][row][ch * 8]) = v;
      }
    }
  }
  __syncthreads();
  // ---- (G - diag) vc, both branches: wave -> rows 32 (wave & 3), columns 32 (wave >> 2)
  const int wr = wave & 3, wc = wave >> 2, r = lane & 31, h = lane >> 5;
  f32x16 acc[2];
#pragma unroll
  for (int br = 0; br < 2; ++br)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[br][e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
#pragma unroll
    for (int br = 0; br < 2; ++br) {
      const bf16x8 fa = *reinterpret_cast<const bf16x8*>(&s_a[br][wr * 32 + r][ks * 16 + h * 8]);
      const bf16x8 fb = *reinterpret_cast<const bf16x8*>(&s_b[br][wc * 32 + r][ks * 16 + h * 8]);
      acc[br] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[br], 0, 0, 0);
    }
  __syncthreads();                                               // every wave is done with the operands
#pragma unroll
  for (int br = 0; br < 2; ++br)
#pragma unroll
    for (int e = 0; e < 16; ++e)
      s_c[br][vc_c32_row(wr * 32, e, h)][wc * 32 + r] = acc[br][e];
  __syncthreads();
  // ---- elementwise terms: thread -> 4 fixed columns, rows tid / 16 + 32 i
  const VcGradK k = vc_grad_k(gcoef, sim_coeff, std_coeff, cov_coeff, B, D, cfg_batch);
  const int c4 = tid & 15, jc = j0 + 4 * c4;
  if (jc >= D) return;                                           // D % 4 == 0: the four columns are in or out together
  float mu[2][4], av[2][4];
#pragma unroll
  for (int br = 0; br < 2; ++br) {
    const vc_f32x4 m = *reinterpret_cast<const vc_f32x4*>(colstats + (size_t)br * D + jc);
    const vc_f32x4 m2 = *reinterpret_cast<const vc_f32x4*>(colstats + (size_t)(2 + br) * D + jc);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      mu[br][c] = m[c];
      av[br][c] = vc_col_av(k, m2[c], B, D);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = (tid >> 4) + 32 * i;
    if (b >= B) continue;
    const vc_f32x4 xv = *reinterpret_cast<const vc_f32x4*>(x + (size_t)b * ld + jc);
    const vc_f32x4 yv = *reinterpret_cast<const vc_f32x4*>(y + (size_t)b * ld + jc);
    const vc_f32x4 cx = *reinterpret_cast<const vc_f32x4*>(&s_c[0][b][4 * c4]);
    const vc_f32x4 cy = *reinterpret_cast<const vc_f32x4*>(&s_c[1][b][4 * c4]);
    const float gdx = gdiag[b], gdy = gdiag[128 + b];
    vc_f32x4 ox, oy;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = k.repr_k * (xv[c] - yv[c]);
      const float vx = xv[c] - mu[0][c], vy = yv[c] - mu[1][c];
      ox[c] = d + av[0][c] * vx + k.cck * (cx[c] + gdx * vx);
      oy[c] = -d + av[1][c] * vy + k.cck * (cy[c] + gdy * vy);
    }
    *reinterpret_cast<vc_f32x4*>(gx + (size_t)b * ldg + jc) = ox;
    *reinterpret_cast<vc_f32x4*>(gy + (size_t)b * ldg + jc) = oy;
  }
}

// ---- the same two products for batch > 128 on the 256 x 256 LDS-DMA tile product (g2_product) -------------------------
// One upper-triangular 256 x 256 tile of one D-slice of G per workgroup (grid: tiles x slices x branches), written once
// to the slice's own Gram (fixed-order sum over the slices in vicreg_gconv256_kernel: deterministic).
__global__ __launch_bounds__(G2_THREADS, 2) void vicreg_bgram256_kernel(const unsigned short* __restrict__ Xc_x,
                                                                        const unsigned short* __restrict__ Xc_y,
                                                                        float* __restrict__ Gp, int D, int Kpad, int nt,
                                                                        int ksplit) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_g2[];
  const int wr = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >> 2;   // which half of the tile's rows this wave holds
  int ti, tj;
  vc_tri_tile(blockIdx.x, nt, ti, tj);
  const int branch = blockIdx.z;
  const unsigned short* Xc = branch ? Xc_y : Xc_x;
  float* Gb = Gp + ((size_t)blockIdx.y * 2 + branch) * Kpad * Kpad;
  const int kbeg = blockIdx.y * ksplit, kend = min(kbeg + ksplit, D);     // D % 64 == 0, ksplit % 64 == 0 (host)
  vc_f32x4 acc[8][4];
  vc_zero(acc);
  g2_product(Xc, (unsigned)D, Kpad, ti * G2_T, Xc, (unsigned)D, Kpad, tj * G2_T, kbeg, (kend - kbeg) / G2_BK, s_g2, acc);
  // rows of the tile through LDS (g2_stage_store): 16-byte stores, 1 KB per wave and row.  Only the upper triangle of
  // tiles is written; vicreg_gconv256_kernel mirrors it when it folds the slices.
  float* s_c = reinterpret_cast<float*>(s_g2);
  const int tid = threadIdx.x, c4 = tid & 63, j0 = tj * G2_T + 4 * c4;
  for (int half = 0; half < 2; ++half) {
    if (wr == half) g2_stage_store(s_c, acc);
    __syncthreads();
    for (int i = 0; i < 16; ++i) {
      const int rl = 8 * i + (tid >> 6);
      const int row = ti * G2_T + 128 * half + rl;
      if (row < Kpad && j0 < Kpad)                               // Kpad % 4 == 0: the four columns are in or out together
        *reinterpret_cast<vc_f32x4*>(Gb + (size_t)row * Kpad + j0) = g2_stage_read(s_c, rl);
    }
    __syncthreads();
  }
}

// G = sum over the D-slices of their partial Grams, in slice order, for the upper-triangular 256 x 256 tiles
// vicreg_bgram256_kernel wrote; one 64 x 64 block per workgroup: bf16 with the diagonal taken out (gdiag, see
// vicreg_gconv_kernel), written in place and -- off the diagonal tiles -- mirrored through an LDS transpose.
__global__ __launch_bounds__(256) void vicreg_gconv256_kernel(const float* __restrict__ Gp, unsigned short* __restrict__ Gb,
                                                              float* __restrict__ gdiag, int Kpad, int nsplit, int nt,
                                                              double* __restrict__ g2part /* [2][gridDim.x] or null */) {
  __shared__ float s_t[64][65];
  __shared__ double s_sq[4];
  int ti, tj;
  vc_tri_tile(blockIdx.x >> 4, nt, ti, tj);
  const int sub = blockIdx.x & 15, branch = blockIdx.y;
  const int r0 = ti * G2_T + (sub >> 2) * 64, c0 = tj * G2_T + (sub & 3) * 64;
  const bool inside = r0 < Kpad && c0 < Kpad;                    // Kpad % 64 == 0: a block is inside or outside
  const size_t plane = (size_t)Kpad * Kpad, n2 = 2 * plane;
  const int tid = threadIdx.x, cc = tid & 63;
  double sq = 0.0;                                               // sum of G_ab^2 over the block (the diagonal included)
  if (inside)
    for (int rr = tid >> 6; rr < 64; rr += 4) {
      const int row = r0 + rr, col = c0 + cc;
      const size_t i = (size_t)branch * plane + (size_t)row * Kpad + col;
      float v = 0.0f;
      VC_FOLD_SLICES(v, Gp, n2, i, nsplit);
      sq += (double)v * (double)v;
      if (row == col) { gdiag[(size_t)branch * Kpad + row] = v; v = 0.0f; }
      Gb[i] = f2bf(v);
      s_t[rr][cc] = v;
    }
  if (g2part) {
    for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d, 64);
    if ((tid & 63) == 0) s_sq[tid >> 6] = sq;
  }
  __syncthreads();
  if (g2part && tid == 0)                                        // tiles above the diagonal stand for their mirror image too
    g2part[(size_t)branch * gridDim.x + blockIdx.x] = (ti == tj ? 1.0 : 2.0) * (((s_sq[0] + s_sq[1]) + s_sq[2]) + s_sq[3]);
  if (inside && ti != tj)
    for (int rr = tid >> 6; rr < 64; rr += 4)                    // row c0 + rr of the mirror image, columns r0 + cc
      Gb[(size_t)branch * plane + (size_t)(c0 + rr) * Kpad + r0 + cc] = f2bf(s_t[cc][rr]);
}

// One 256 (batch rows) x 256 (features) tile of gx (branch 0) or gy (branch 1) per workgroup: (G - diag) vc on the
// matrix cores, then the elementwise terms (the epilogue of vicreg_grad_kernel, one branch) on the rows staged through
// LDS (g2_stage_store / g2_stage_read): 16-byte accesses to x, y and the gradient.
__global__ __launch_bounds__(G2_THREADS, 2) void vicreg_grad256_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const unsigned short* __restrict__ Xt_x,
    const unsigned short* __restrict__ Xt_y, const unsigned short* __restrict__ Gb, const float* __restrict__ gdiag,
    const float* __restrict__ colstats, const VcCot gcoef, float* __restrict__ gx, float* __restrict__ gy,
    int B, int D, int Kpad, int cfg_batch, float sim_coeff, float std_coeff, float cov_coeff, size_t ld, size_t ldg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_g2[];
  const int wr = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >> 2;   // which half of the tile's rows this wave holds
  const int col0 = blockIdx.x * G2_T, row0 = blockIdx.y * G2_T, branch = blockIdx.z;
  const VcGradK k = vc_grad_k(gcoef, sim_coeff, std_coeff, cov_coeff, B, D, cfg_batch);
  vc_f32x4 acc[8][4];
  vc_zero(acc);
  g2_product(Gb + (size_t)branch * Kpad * Kpad, (unsigned)Kpad, Kpad, row0, branch ? Xt_y : Xt_x, (unsigned)Kpad, D, col0, 0,
             Kpad / G2_BK, s_g2, acc);
  const float repr_k = branch ? -k.repr_k : k.repr_k;
  float* gout = branch ? gy : gx;
  const float* own = branch ? y : x;
  float* s_c = reinterpret_cast<float*>(s_g2);
  const int tid = threadIdx.x, c4 = tid & 63, j0 = col0 + 4 * c4;
  float mu[4], av[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = j0 + c;
    mu[c] = 0.f; av[c] = 0.f;
    if (j < D) {
      mu[c] = colstats[(size_t)branch * D + j];
      av[c] = vc_col_av(k, colstats[(size_t)(2 + branch) * D + j], B, D);
    }
  }
  const bool vec = (D & 3) == 0 && ((ld | ldg) & 3) == 0 && j0 + 3 < D;   // (16-byte aligned bases: checked by the caller)
  for (int half = 0; half < 2; ++half) {
    if (wr == half) g2_stage_store(s_c, acc);
    __syncthreads();
    for (int i = 0; i < 16; ++i) {
      const int rl = 8 * i + (tid >> 6);                       // row inside the half
      const int b = row0 + 128 * half + rl;
      if (b >= B) continue;
      const vc_f32x4 cv = g2_stage_read(s_c, rl);
      const float gd = gdiag[(size_t)branch * Kpad + b];
      const size_t idx = (size_t)b * ld + j0, odx = (size_t)b * ldg + j0;
      if (vec) {
        const vc_f32x4 xv = *reinterpret_cast<const vc_f32x4*>(x + idx), yv = *reinterpret_cast<const vc_f32x4*>(y + idx);
        vc_f32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float v = (branch ? yv[c] : xv[c]) - mu[c];
          o[c] = repr_k * (xv[c] - yv[c]) + av[c] * v + k.cck * (cv[c] + gd * v);
        }
        *reinterpret_cast<vc_f32x4*>(gout + odx) = o;
      } else {
        for (int c = 0; c < 4; ++c) {
          if (j0 + c >= D) break;
          const float v = own[idx + c] - mu[c];
          gout[odx + c] = repr_k * (x[idx + c] - y[idx + c]) + av[c] * v + k.cck * (cv[c] + gd * v);
        }
      }
    }
    __syncthreads();
  }
}

void vicreg_launch_batch_gram(const VicregWs& w, char* ws, int D, hipStream_t stream, bool squares) {
  float* G = (float*)(ws + w.bgram);
  const int bt = w.Kpad / GT, npair = bt * (bt + 1) / 2;
  const size_t lds256 = 2 * (size_t)G2_BUF_BYTES;
  const int bt2 = (w.Kpad + G2_T - 1) / G2_T;
  unsigned short* Gb = (unsigned short*)(ws + w.bgram16);
  float* gdiag = (float*)(ws + w.gdiag);
  double* g2part = squares ? (double*)(ws + w.g2part) : nullptr;
  if (w.b256) {
    (void)hipFuncSetAttribute((const void*)vicreg_bgram256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds256);
    hipLaunchKernelGGL(vicreg_bgram256_kernel, dim3(bt2 * (bt2 + 1) / 2, w.nsplit, 2), dim3(G2_THREADS), lds256, stream,
                       (const unsigned short*)(ws + w.xc_x), (const unsigned short*)(ws + w.xc_y), G, D, w.Kpad, bt2, w.ksplit);
    hipLaunchKernelGGL(vicreg_gconv256_kernel, dim3(16 * (bt2 * (bt2 + 1) / 2), 2), dim3(256), 0, stream, G, Gb, gdiag, w.Kpad,
                       w.nsplit, bt2, g2part);
  } else {
    hipLaunchKernelGGL(vicreg_bgram_kernel, dim3(npair, w.nsplit, 2), dim3(256), 0, stream, (const unsigned short*)(ws + w.xc_x),
                       (const unsigned short*)(ws + w.xc_y), G, D, w.Kpad, bt, w.ksplit);
    hipLaunchKernelGGL(vicreg_gconv_kernel, dim3(w.ng2 / 2), dim3(256), 0, stream, G, Gb, gdiag, w.Kpad, w.nsplit, g2part);
  }
}

int vicreg_backward_ld(const float* x, const float* y, long long ld, const VcCot gcoef, float* gx, float* gy,
                       long long ldg, void* workspace, long long workspace_bytes, int B, int D, int cfg_batch,
                       float sim_coeff, float std_coeff, float cov_coeff, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !y || !gx || !gy || !workspace || B < 2 || D < 8 || (D & 7) || cfg_batch < 2 || ld < D || ldg < D)
    return IAS_ERR_ARG;
  // the 256-tile epilogue moves 16 bytes per access: strided views must keep that alignment
  if ((ld != D || ldg != D) && ((((size_t)x | (size_t)y | (size_t)gx | (size_t)gy) & 15) || ((ld | ldg) & 3))) return IAS_ERR_ARG;
  const VicregWs w = vicreg_ws(B, D);
  if ((size_t)workspace_bytes < w.total) return IAS_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  const int bt = w.Kpad / GT;
  if (w.Kpad % GT) return IAS_ERR_UNSUPPORTED;
  const bool b256 = w.b256;
  const size_t lds256 = 2 * (size_t)G2_BUF_BYTES;
  const int bt2 = (w.Kpad + G2_T - 1) / G2_T;
  if (!w.dual) vicreg_launch_batch_gram(w, ws, D, stream, false);   // (batch-side forward: G and its diagonal are in place)
  unsigned short* Gb = (unsigned short*)(ws + w.bgram16);
  float* gdiag = (float*)(ws + w.gdiag);
  if (b256) {
    (void)hipFuncSetAttribute((const void*)vicreg_grad256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds256);
    hipLaunchKernelGGL(vicreg_grad256_kernel, dim3((D + G2_T - 1) / G2_T, bt2, 2), dim3(G2_THREADS), lds256, stream, x, y,
                       (const unsigned short*)(ws + w.xt_x), (const unsigned short*)(ws + w.xt_y), Gb, gdiag,
                       (const float*)(ws + w.colstats), gcoef, gx, gy, B, D, w.Kpad, cfg_batch, sim_coeff, std_coeff, cov_coeff,
                       (size_t)ld, (size_t)ldg);
  } else if (w.Kpad == 128 && !((((size_t)x | (size_t)y | (size_t)gx | (size_t)gy) & 15) || ((ld | ldg) & 3))) {
    (void)hipFuncSetAttribute((const void*)vicreg_grad128_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, G1_LDS_BYTES);
    hipLaunchKernelGGL(vicreg_grad128_kernel, dim3((D + G1_COLS - 1) / G1_COLS), dim3(512), G1_LDS_BYTES, stream, x, y,
                       (const unsigned short*)(ws + w.xt_x), (const unsigned short*)(ws + w.xt_y), Gb, gdiag,
                       (const float*)(ws + w.colstats), gcoef, gx, gy, B, D, cfg_batch, sim_coeff, std_coeff, cov_coeff,
                       (size_t)ld, (size_t)ldg);
  } else {
    hipLaunchKernelGGL(vicreg_grad_kernel, dim3((D + GT - 1) / GT, bt, 2), dim3(256), 0, stream, x, y,
                       (const unsigned short*)(ws + w.xt_x), (const unsigned short*)(ws + w.xt_y), Gb, gdiag,
                       (const float*)(ws + w.colstats), gcoef, gx, gy, B, D, w.Kpad, cfg_batch, sim_coeff, std_coeff, cov_coeff,
                       (size_t)ld, (size_t)ldg);
  }
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
