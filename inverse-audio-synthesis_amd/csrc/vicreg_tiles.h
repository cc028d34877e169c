// What more than one of the VICReg kernel files needs (vicreg_kernels.hip: forward and C ABI; vicreg_dxd_kernels.hip:
// the feature-side D x D Gram; vicreg_grad_kernels.hip: the batch-side B x B Gram and the backward): the fragment types
// and tile constants, the two tile products on the matrix cores, the enumeration of the upper-triangular tiles of a
// symmetric matrix, and the small accumulator helpers.  Each defined once, before its first use.
#pragma once
#include "ias_common.h"
#include <hip/hip_bf16.h>

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float vc_f32x4;

#define GT 128            // gram output tile (GT x GT)
#define GK 64             // k-chunk staged per iteration
#define GLD (GK + 8)      // LDS row stride in bf16 (144 B: breaks the 128-B row bank aliasing)

__device__ __forceinline__ unsigned short f2bf(float f) {
  return __builtin_bit_cast(unsigned short, __float2bfloat16(f));
}

typedef __attribute__((address_space(3))) void gram_lds_void;
typedef const __attribute__((address_space(1))) void gram_glb_void;

__device__ __forceinline__ void gp_lds_read_b128(bf16x8& dst, unsigned lds_addr) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(lds_addr) : "memory");
}
// the wait that makes two asm-loaded fragments usable: they pass through it, so no consumer can be scheduled above it
__device__ __forceinline__ void gp_lds_wait(bf16x8& a, bf16x8& b) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b) : : "memory");
}

// linear index over the tiles on or above the diagonal of an ntile x ntile grid, row by row -> (ti, tj), ti <= tj
__device__ __forceinline__ void vc_tri_tile(int item, int ntile, int& ti, int& tj) {
  int t = item;
  ti = 0;
  int rowlen = ntile;
  while (t >= rowlen) { t -= rowlen; --rowlen; ++ti; }
  tj = ti + t;
}

// ---- the accumulators of the two tile products ------------------------------------------------------------------------
// C layout of a 32 x 32 block (v_mfma_f32_32x32x16_bf16) whose first row is row0: element e of the lane with
// h = lane >> 5 is in this row, in column lane & 31.  (A 16 x 16 block of v_mfma_f32_16x16x32_bf16: row 4 (lane >> 4) + e,
// column lane & 15.)  One sum from left to right, row0 first: with the block's part summed on its own the compiler folds
// fewer of the constant terms into the address offsets of vicreg_grad_kernel's epilogue (60 more 64-bit additions).
__device__ __forceinline__ int vc_c32_row(int row0, int e, int h) { return row0 + (e & 3) + 8 * (e >> 2) + 4 * h; }

__device__ __forceinline__ void vc_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
}
__device__ __forceinline__ void vc_zero(vc_f32x4 (&acc)[8][4]) {
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = (vc_f32x4){0.f, 0.f, 0.f, 0.f};
}

// ---- 128 x 128 tile product, operands staged through registers ------------------------------------------------------
// acc += A[row0 .. row0+127][k] B[col0 .. col0+127][k]^T over k in [kbeg, kend) (kbeg a multiple of GK, kend of 8), A / B bf16 row-major
// with row strides lda / ldb; rows >= arows / brows and k >= kend read as zero.  256 threads as 2 x 2 waves, 64 x 64 each
// (acc[m][n]: the 32 x 32 block at rows wr*64 + 32 m, columns wc*64 + 32 n of the tile).  The k loop is double-buffered:
// the next 64-deep chunk of both panels is fetched into registers while the matrix cores work on the current one and
// written to the other LDS buffer afterwards (one barrier per chunk).
__device__ __forceinline__ void vc_tile_product(const unsigned short* __restrict__ A, size_t lda, int arows,
                                                const unsigned short* __restrict__ Bm, size_t ldb, int brows, int row0,
                                                int col0, int kbeg, int kend, unsigned short (*s_a)[GT][GLD],
                                                unsigned short (*s_b)[GT][GLD], f32x16 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  // one 64-deep chunk of A (rows row0..+127) and B (rows col0..+127): 128 rows x 128 B each, 16 B per thread x 4
  uint4 sta[4], stb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (tid >> 3) + 32 * i, ch = tid & 7;
      sta[i] = make_uint4(0, 0, 0, 0); stb[i] = make_uint4(0, 0, 0, 0);
      const bool kin = k0 + ch * 8 + 8 <= kend;            // (kend % 8 == 0; a last chunk shorter than GK reads zeros)
      if (kin && row0 + rr < arows) sta[i] = *reinterpret_cast<const uint4*>(A + (size_t)(row0 + rr) * lda + k0 + ch * 8);
      if (kin && col0 + rr < brows) stb[i] = *reinterpret_cast<const uint4*>(Bm + (size_t)(col0 + rr) * ldb + k0 + ch * 8);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (tid >> 3) + 32 * i, ch = tid & 7;
      *reinterpret_cast<uint4*>(&s_a[buf][rr][ch * 8]) = sta[i];
      *reinterpret_cast<uint4*>(&s_b[buf][rr][ch * 8]) = stb[i];
    }
  };
  __syncthreads();                         // the buffers may still be read by a previous product of this workgroup
  fetch(kbeg);
  commit(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += GK) {
    const bool more = k0 + GK < kend;
    if (more) fetch(k0 + GK);              // in flight while the matrix cores work on this chunk
#pragma unroll
    for (int ks = 0; ks < GK / 16; ++ks) {
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
        fa[m] = *reinterpret_cast<const bf16x8*>(&s_a[buf][wr * 64 + m * 32 + r][ks * 16 + h * 8]);
#pragma unroll
      for (int n = 0; n < 2; ++n)
        fb[n] = *reinterpret_cast<const bf16x8*>(&s_b[buf][wc * 64 + n * 32 + r][ks * 16 + h * 8]);
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
    if (more) commit(buf ^ 1);             // the other buffer: nobody reads it during this chunk
    __syncthreads();
    buf ^= 1;
  }
}

// ---- 256 x 256 tile product for deep contractions (batch > 128: BASELINE configs[3], global batch 1024) ---------------
// The 128 x 128 product above is bound by the LDS store path: 8 ds_write_b128 per thread and 64-deep chunk = 832 LDS
// cycles per CU against 1024 MFMA cycles, on top of 512 cycles of fragment reads (profiles/r03b_kstats_vicreg1024.csv:
// 0.29 of the bf16 peak).  Here:
//   * 256 x 256 tile per workgroup, 8 waves as 2 (rows) x 4 (columns), 128 x 64 per wave on v_mfma_f32_16x16x32_bf16
//     (32 accumulator tiles = 128 VGPRs): 24 fragment reads feed 64 MFMAs per wave and 64-deep K-tile (reads 37 % of the
//     MFMA time instead of 50 %, and half the staged bytes per flop);
//   * both operands' K-tiles (256 rows x 128 B each) come in by LDS-DMA (global_load_lds, 16 B per lane: no VGPRs, no
//     ds_write) into two 64 KB buffers, K-tile kt + 1 requested in pieces between the MFMA groups of K-tile kt;
//   * LDS image: row r at r * 128 B, its 16-byte granule g at slot g ^ ((r >> 1) & 7) -- lane-linear for the DMA (the
//     SOURCE address is permuted), conflict-free for the 16 x 32 fragment reads (ds_read_b128 lane groups);
//   * fragments by inline-asm ds_read_b128, double-buffered in registers: the reads of the next (k-step, row half) are
//     issued before the 16 MFMAs of the current one and waited for with a counted lgkmcnt; one raw barrier per K-tile.
#define G2_T 256
#define G2_BK 64
#define G2_THREADS 512
#define G2_TILE_BYTES (G2_T * G2_BK * 2)
#define G2_BUF_BYTES (2 * G2_TILE_BYTES)

#define G2_WAIT(N, X, Y) do { asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(Y[0]), "+v"(Y[1]), "+v"(Y[2]), "+v"(Y[3]) : : "memory"); } while (0)

// acc[8][4] (16 x 16 tiles: rows wr*128 + 16 m + 4 (lane >> 4) + reg, columns wc*64 + 16 n + (lane & 15)) +=
// A[row0 .. +255][k] B[col0 .. +255][k]^T over k in [k0, k0 + 64 nkt), A / B bf16 row-major with row strides lda / ldb
// (elements; every offset < 2^31).  Rows >= arows / brows repeat the last valid row: mask them in the epilogue.
// s_g2: the workgroup's 128 KB staging area; on return every wave has passed the barrier behind the last K-tile.
__device__ __forceinline__ void g2_product(const unsigned short* __restrict__ A, unsigned lda, int arows, int row0,
                                           const unsigned short* __restrict__ Bm, unsigned ldb, int brows, int col0,
                                           int k0, int nkt, unsigned char* s_g2, vc_f32x4 (&acc)[8][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int r = lane & 15, q = lane >> 4;
  // ---- LDS-DMA pieces: a K-tile is 64 pieces of 1 KB (8 rows x 128 B), piece = wave + 8 i; pieces 0..31 operand A
  unsigned src_off[8];            // element offset of this lane's 16 bytes of piece i at K-tile 0
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int piece = wave + 8 * i, pp = piece & 31;
    const int row = 8 * pp + (lane >> 3);
    const int g = (lane & 7) ^ ((row >> 1) & 7);
    int grow = (i >= 4 ? col0 : row0) + row;
    const int lim = i >= 4 ? brows : arows;
    grow = grow < lim ? grow : lim - 1;
    src_off[i] = (unsigned)grow * (i >= 4 ? ldb : lda) + (unsigned)(k0 + g * 8);
  }
  auto request = [&](int kt, int i) {
    const int piece = wave + 8 * i, pp = piece & 31;
    unsigned char* dst = s_g2 + (kt & 1) * G2_BUF_BYTES + (i >= 4 ? G2_TILE_BYTES : 0) + pp * 1024;
    __builtin_amdgcn_global_load_lds((gram_glb_void*)((i >= 4 ? Bm : A) + (size_t)src_off[i] + (size_t)kt * G2_BK),
                                     (gram_lds_void*)dst, 16, 0, 0);
  };
  // ---- fragment addresses
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)s_g2;
  const unsigned sw0 = (unsigned)((q ^ ((r >> 1) & 7)) << 4), sw1 = (unsigned)(((4 + q) ^ ((r >> 1) & 7)) << 4);
  const unsigned a_lane = (unsigned)((wr * 128 + r) * 128), b_lane = (unsigned)(G2_TILE_BYTES + (wc * 64 + r) * 128);

  // K-tile 0
#pragma unroll
  for (int i = 0; i < 8; ++i) request(0, i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  bf16x8 fa[2][4], fb[2][4];
  for (int kt = 0; kt < nkt; ++kt) {
    const unsigned buf = lds0 + (unsigned)((kt & 1) * G2_BUF_BYTES);
    const bool more = kt + 1 < nkt;
    auto read_a = [&](bf16x8 (&dst)[4], int ks, int mq) {
#pragma unroll
      for (int m = 0; m < 4; ++m) gp_lds_read_b128(dst[m], buf + a_lane + (ks ? sw1 : sw0) + (unsigned)(mq * 8192 + m * 2048));
    };
    auto read_b = [&](bf16x8 (&dst)[4], int ks) {
#pragma unroll
      for (int n = 0; n < 4; ++n) gp_lds_read_b128(dst[n], buf + b_lane + (ks ? sw1 : sw0) + (unsigned)(n * 2048));
    };
    auto mfma16 = [&](const bf16x8 (&Af)[4], const bf16x8 (&Bf)[4], int mq) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[mq * 4 + m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Af[m], Bf[n], acc[mq * 4 + m][n], 0, 0, 0);
    };
    read_a(fa[0], 0, 0);
    read_b(fb[0], 0);
    // unit 0: (k-step 0, rows 0..63 of the wave)
    read_a(fa[1], 0, 1);
    if (more) { request(kt + 1, 0); request(kt + 1, 1); request(kt + 1, 2); }
    G2_WAIT(4, fa[0], fb[0]);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(fa[0], fb[0], 0);
    __builtin_amdgcn_sched_barrier(0);
    // unit 1: (k-step 0, rows 64..127)
    read_a(fa[0], 1, 0);
    read_b(fb[1], 1);
    if (more) { request(kt + 1, 3); request(kt + 1, 4); request(kt + 1, 5); }
    G2_WAIT(8, fa[1], fb[0]);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(fa[1], fb[0], 1);
    __builtin_amdgcn_sched_barrier(0);
    // unit 2: (k-step 1, rows 0..63)
    read_a(fa[1], 1, 1);
    if (more) { request(kt + 1, 6); request(kt + 1, 7); }
    G2_WAIT(4, fa[0], fb[1]);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(fa[0], fb[1], 0);
    __builtin_amdgcn_sched_barrier(0);
    // unit 3: (k-step 1, rows 64..127)
    G2_WAIT(0, fa[1], fb[1]);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(fa[1], fb[1], 1);
    __builtin_amdgcn_sched_barrier(0);
    // K-tile kt + 1 has landed (this wave's pieces), every wave is done reading K-tile kt
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
}
