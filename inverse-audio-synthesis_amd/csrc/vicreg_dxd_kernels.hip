// VICReg covariance term from the feature side: C = Xt Xt^T (D x D, contracted over the batch) on the matrix cores, never
// stored -- each upper-triangular tile is squared, summed without its diagonal elements (x 2 above the diagonal) and
// reduced to one fp64 partial, which vicreg_finish_kernel (vicreg_kernels.hip) adds up.  Xt [D][Kpad] bf16 is the centred,
// transposed, zero-padded matrix the column pass leaves.  The product takes this side only where the batch side
// (vicreg_grad_kernels.hip) does not apply: padded batch > D, or D not a multiple of 8; the diagnostic library takes it
// on request (ias_vicreg_set_form(0), IAS_VICREG_DXD=1: bench.py times it for `roofline.dxd`).  Which kernel by shape:
//   vicreg_gram_pair_kernel   Kpad == 128 (batch <= 128): a pair of row panels in registers, column panels streamed past
//   vicreg_gram256_kernel     Kpad > 128, D >= 256, D Kpad < 2^31: 256 x 256 tiles by LDS-DMA (g2_product)
//   vicreg_gram_kernel        Kpad > 128 otherwise (D < 256, or IAS_VICREG_GRAM128=1): 128 x 128 tiles (vc_tile_product)
#include "vicreg_tiles.h"
#include "vicreg_internal.h"

// One upper-triangular 128x128 tile of C = Xt Xt^T per workgroup and branch (blockIdx.y); partial[tile] = sum of
// squares of the tile's off-diagonal elements (x2 for tiles above the diagonal).  Any contraction depth.
__global__ __launch_bounds__(256, 2) void vicreg_gram_kernel(const unsigned short* __restrict__ Xt_x,
                                                             const unsigned short* __restrict__ Xt_y,
                                                             double* __restrict__ part_x, double* __restrict__ part_y,
                                                             int D, int Kpad, int ntile) {
  __shared__ __attribute__((aligned(16))) unsigned short s_a[2][GT][GLD];
  __shared__ __attribute__((aligned(16))) unsigned short s_b[2][GT][GLD];
  __shared__ double s_part[4];
  const unsigned short* Xt = blockIdx.y ? Xt_y : Xt_x;
  double* partials = blockIdx.y ? part_y : part_x;
  int ti, tj;
  vc_tri_tile(blockIdx.x, ntile, ti, tj);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;      // 2 x 2 waves, 64 x 64 each
  const int r = lane & 31, h = lane >> 5;

  f32x16 acc[2][2];
  vc_zero(acc);
  vc_tile_product(Xt, (size_t)Kpad, D, Xt, (size_t)Kpad, D, ti * GT, tj * GT, 0, Kpad, s_a, s_b, acc);

  // epilogue: sum of squares
  float s = 0.f;
  const bool diag_tile = (ti == tj);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float v = acc[m][n][e];
        if (diag_tile) {
          const int row = vc_c32_row(wr * 64 + m * 32, e, h);
          const int col = wc * 64 + n * 32 + r;
          if (row != col) s = fmaf(v, v, s);
        } else {
          s = fmaf(v, v, s);
        }
      }
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) s_part[wave] = (double)s;
  __syncthreads();
  if (tid == 0) {
    const double tot = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    partials[blockIdx.x] = diag_tile ? tot : 2.0 * tot;
  }
}

// ---- Gram for a contraction depth of 128 (batch <= 128, BASELINE configs[2]) -----------------------------------
// At K = 128 a 128 x 128 tile is only 32 MFMAs per wave: what bounds the kernel is the panel traffic L2 -> LDS
// (~30 B/clk per CU at best), not the matrix cores.  So a workgroup keeps a PAIR of row panels (256 rows x K = 128) in
// registers as A fragments (128 VGPRs per lane) and streams the column panels past them: one 32 KB panel fetched feeds
// 64 MFMAs per wave (two tiles), 16 B/clk at full matrix rate.  The panels come in by LDS-DMA (no VGPR staging) into a
// ring of four 32 KB slots (the pair of panels being read + the pair landing); one raw s_barrier per PAIR of steps.  LDS image of a panel:
// [128 rows][16 granules of 16 B], granule g of row r at slot g ^ (r & 15) -- conflict-free for the fragment reads
// (16 consecutive rows, same granule) and lane-linear for the DMA once the SOURCE address is permuted the same way.
// Tiles below the diagonal of a pair (2p+1, 2p) are computed and given weight 0 (1.5 % of the work).
#define GP_RING 4
#define GP_PANEL_BYTES (GT * 128 * 2)

// A step = one column panel tj streamed past the row-panel pair p of one branch, tj = 2p .. ntile-1.  A work item is a
// run of at most GP_CH consecutive steps of ONE pair: (branch, p, chunk), enumerated branch-major, p-major.  One
// workgroup per item (235 - 260 items at D = 8192: one resident round of one 128 KB-LDS workgroup per CU).
#define GP_CH 10
__device__ __forceinline__ void gp_item(int item, int ntile, int& p, int& c) {
  p = 0;
  for (;;) {
    const int nc = (ntile - 2 * p + GP_CH - 1) / GP_CH;
    if (item < nc) break;
    item -= nc; ++p;
  }
  c = item;
}
static int gp_nitems(int ntile) {
  int n = 0;
  for (int p = 0; 2 * p < ntile; ++p) n += (ntile - 2 * p + GP_CH - 1) / GP_CH;
  return n;
}

#ifdef GP_STAMPS
// Diagnostic build only (scripts/diag): s_memtime stamps of wave 0 of every workgroup, into a buffer of their own.
__device__ unsigned long long* g_gp_stamps = nullptr;
extern "C" int ias_vicreg_debug_set_stamps(unsigned long long* p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_gp_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#define GPSTAMP(i) do { if (g_gp_stamps && (threadIdx.x & 63) == 0) g_gp_stamps[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 32 + (i)] = __builtin_amdgcn_s_memtime(); if (g_gp_stamps && (threadIdx.x & 63) == 0 && (i) == 0) g_gp_stamps[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 32 + 31] = __builtin_amdgcn_s_getreg(6 << 11 | 4 << 6 | 4); } while (0)
#else
#define GPSTAMP(i) do {} while (0)
#endif

#define GP_THREADS 512      // 8 waves, two per SIMD: one wave's square-sum epilogue runs beside its partner's MFMAs
__global__ __launch_bounds__(GP_THREADS, 2) void vicreg_gram_pair_kernel(const unsigned short* __restrict__ Xt_x,
                                                                         const unsigned short* __restrict__ Xt_y,
                                                                         double* __restrict__ part_x,
                                                                         double* __restrict__ part_y, int D, int ntile,
                                                                         int nitems) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_ring[];   // GP_RING x 32 KB
  __shared__ double s_part[GP_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;       // wave tile: rows wr*64 .. +63 of the 256-row pair, columns wc*64 .. +63
  const int r = lane & 31, h = lane >> 5;
  // XCD-aware placement (speed only): consecutive block indices are dealt round-robin over the 8 XCDs, each with its own
  // 4 MB L2.  Blocks with (blockIdx % 8) < 4 work on branch x, the others on branch y, so that an XCD's L2 has to hold
  // only ONE of the two 2 MB matrices -- with both in every L2 a third of the panel requests missed it and the ring
  // filled at the Infinity-Cache rate (measured: 1750 of every 3650 cycles per step spent waiting for the panel).
  const int xslot = blockIdx.x & 7, branch = xslot >> 2;
  const int item = (blockIdx.x >> 3) * 4 + (xslot & 3);
  if (item >= nitems) return;
  const unsigned short* Xt = branch ? Xt_y : Xt_x;
  int p, c;
  gp_item(item, ntile, p, c);
  const int tj0 = 2 * p + c * GP_CH, nsteps = min(GP_CH, ntile - tj0);
  const bool ragged = (D % GT) != 0;

  // panel tj -> ring slot: 4 LDS-DMA instructions per wave (1 KB = 4 rows each); rows beyond D repeat row D - 1
  // (as columns they are masked in the epilogue, as rows of A they are zeroed below)
  auto request_piece = [&](int tj, int slot_i, int i) {
    unsigned char* slot = s_ring + slot_i * GP_PANEL_BYTES;
    const int row = wave * 16 + i * 4 + (lane >> 4);          // row of the panel this lane's 16 bytes belong to
    const int g = (lane & 15) ^ (row & 15);                    // source granule for LDS slot (lane & 15)
    int grow = tj * GT + row;
    grow = grow < D ? grow : D - 1;
    __builtin_amdgcn_global_load_lds((gram_glb_void*)(Xt + (size_t)grow * 128 + g * 8),
                                     (gram_lds_void*)(slot + (wave * 16 + i * 4) * 256), 16, 0, 0);
  };
  auto request = [&](int tj, int slot_i) {
#pragma unroll
    for (int i = 0; i < 4; ++i) request_piece(tj, slot_i, i);
  };

  GPSTAMP(0);
  // ---- the pair's own two panels -> ring slots 0, 1 -> A fragments in registers (they are never re-fetched per wave
  // from global memory: 64 KB per workgroup instead of 16 KB x 8 waves x 2)
  request(2 * p, 0);
  request(min(2 * p + 1, ntile - 1), 1);
  // the first two column panels go to slots 2 and 3 at once (step s uses slot (s + 2) % GP_RING): their latency runs
  // beside the A setup instead of after it
  int requested = 0;
  for (; requested < min(nsteps, 2); ++requested) request(tj0 + requested, (requested + 2) % GP_RING);
  if (requested == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (requested == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  bf16x8 fa[2][8];             // rows wr*64 + m*32 + r of the pair (panel q = wr >> 1), [m block][k step]
  {
    const int q = wr >> 1;
    const unsigned char* slot = s_ring + q * GP_PANEL_BYTES;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int prow = (wr & 1) * 64 + m * 32 + r;               // row inside the panel
      const bool ok = (2 * p + q < ntile) && ((2 * p + q) * GT + prow < D);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        bf16x8 v = *reinterpret_cast<const bf16x8*>(slot + prow * 256 + (((ks * 2 + h) ^ (prow & 15)) << 4));
        if (!ok) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = 0;
        }
        fa[m][ks] = v;
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();        // every wave has its fragments: the slots can be reused

  GPSTAMP(1);
  // ---- stream the column panels
  const unsigned ring_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)s_ring;
  for (; requested < min(nsteps, 4); ++requested) request(tj0 + requested, (requested + 2) % GP_RING);   // slots 0, 1 are free now
  float tot = 0.f;
  const int ti = 2 * p + (wr >> 1);    // the row panel this wave's rows belong to
  const int rbase = (wr & 1) * 64;     // first row of this wave inside its row panel

  // The square-sum epilogue of step s runs INSIDE the MFMA stream of step s + 1 (two accumulator sets, ping-pong): eight
  // FMAs behind each group of four MFMAs, which the matrix pipe hides.  The per-step barrier starts both waves of a SIMD
  // on their MFMAs together, so without this the pipe idles while both run their epilogues.
  //   plain   : sum of squares of the previous tile's 64 values per lane (done inside the MFMA stream)
  //   finish  : what is left for the previous tile after the stream: weights, the diagonal of a diagonal tile
  //             (one element per lane and diagonal block), or the fully masked form for the last panel of a ragged D
  auto finish_prev = [&](const f32x16 (&accP)[2][2], float ssP, int tjP) {
    if (!(ti < ntile && tjP >= ti)) return;      // no such row panel / mirror image of a tile counted elsewhere
    float ss = ssP;
    if (ragged && tjP == ntile - 1) {
      ss = 0.f;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int col = wc * 64 + n * 32 + r;
          const bool col_ok = tjP * GT + col < D;
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int row = vc_c32_row(rbase + m * 32, e, h);
            const float v = accP[m][n][e];
            if (col_ok && !(ti == tjP && row == col)) ss = fmaf(v, v, ss);
          }
        }
    } else if (ti == tjP) {
      // element (row, col) of block (m, n) lies on the diagonal iff rbase + m*32 + rowin == wc*64 + n*32 + r
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int rowin = wc * 64 + n * 32 + r - rbase - m * 32;   // row inside the 32 x 32 block, if in [0, 32)
          const int t = rowin - 4 * h;                                // = (e & 3) + 8 (e >> 2) for the lane's element e
          if (rowin >= 0 && rowin < 32 && t >= 0 && (t & 4) == 0) {
            const int esel = (t & 3) + 4 * (t >> 3);
            float v = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) v = (e == esel) ? accP[m][n][e] : v;
            ss = fmaf(-v, v, ss);
          }
        }
    }
    tot += (ti == tjP) ? ss : 2.0f * ss;
  };

  // Two steps per barrier (round 4).  With a barrier per step all eight waves start their 32 MFMAs together and finish
  // together, and the ~1,100 cycles between two streams (barrier, first fragment reads, the rest of the epilogue) leave
  // the matrix cores idle: in-kernel stamps had a step at 3,650 cycles for 2,050 of matrix work, with and without the
  // panel loads.  A barrier now covers a PAIR of steps: the fragments of the second panel are read while the first
  // one's MFMAs run.  Ring: the pair being read (two slots) + the pair landing (two slots); the landing pair is requested
  // in the FIRST step of the pair before (one 1 KB piece per k step), so it has the second step's duration to arrive.
  auto sync_pair = [&](int s, int npanels) {
    // this wave's loads of panels s .. s + npanels - 1 have landed once at most the loads of the later panels requested
    // so far are outstanding (vector memory operations retire in order); the barrier extends that to every wave's part
    // and frees the slots of the pair before
    const int later = requested - (s + npanels);
    if (later >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  // one step: MFMAs of panel s into accC, plain square sums of accP (the previous step) in their shadow; `nreq` panels
  // (0, 1 or 2) are requested on the way, a piece per k step
  auto step = [&](int s, f32x16 (&accC)[2][2], const f32x16 (&accP)[2][2], bool haveP, int nreq) {
    GPSTAMP(2 + 2 * s);
    const int req_tj0 = tj0 + requested, req_slot0 = (requested + 2) % GP_RING;
    const int req_tj1 = req_tj0 + 1, req_slot1 = (requested + 3) % GP_RING;
    requested += nreq;

    // B fragments by inline-asm ds_read_b128: through the compiler's own LDS loads every step would first drain ALL
    // outstanding LDS-DMA (it cannot tell the slot being read from the slots being filled and inserts vmcnt(0)), which
    // serialises the ring.  The reads of k step ks + 1 are issued before the MFMAs of step ks and waited for after them.
    const unsigned slot_a = ring_lds + (unsigned)(((s + 2) % GP_RING) * GP_PANEL_BYTES);
    bf16x8 fb[2][2];    // [ks & 1][n]
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int brow = wc * 64 + n * 32 + r;
      gp_lds_read_b128(fb[0][n], slot_a + (unsigned)(brow * 256 + ((h ^ (brow & 15)) << 4)));
    }
    gp_lds_wait(fb[0][0], fb[0][1]);
    float ssP = 0.f;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      if (ks + 1 < 8) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int brow = wc * 64 + n * 32 + r;
          gp_lds_read_b128(fb[(ks + 1) & 1][n], slot_a + (unsigned)(brow * 256 + ((((ks + 1) * 2 + h) ^ (brow & 15)) << 4)));
        }
      }
      if (ks < 4 ? nreq >= 1 : nreq >= 2) request_piece(ks < 4 ? req_tj0 : req_tj1, ks < 4 ? req_slot0 : req_slot1, ks & 3);
      __builtin_amdgcn_sched_barrier(0);   // keep this k step's MFMAs between the issue of the next reads and their wait
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if (ks == 0) {
            f32x16 z;
#pragma unroll
            for (int e = 0; e < 16; ++e) z[e] = 0.f;
            accC[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m][ks], fb[ks & 1][n], z, 0, 0, 0);
          } else {
            accC[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[m][ks], fb[ks & 1][n], accC[m][n], 0, 0, 0);
          }
        }
      // eight of the previous tile's 64 squares: block (ks >> 1), elements 8 (ks & 1) .. + 7
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = accP[(ks >> 2) & 1][(ks >> 1) & 1][8 * (ks & 1) + e];
        ssP = fmaf(v, v, ssP);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ks + 1 < 8) gp_lds_wait(fb[(ks + 1) & 1][0], fb[(ks + 1) & 1][1]);
    }
    GPSTAMP(3 + 2 * s);
    if (haveP) finish_prev(accP, ssP, tj0 + s - 1);
  };

  f32x16 acc0[2][2], acc1[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc0[m][n][e] = 0.f; acc1[m][n][e] = 0.f; }
  int s = 0;
  for (; s + 1 < nsteps; s += 2) {
    sync_pair(s, 2);
    // the slots of panels s - 2, s - 1 are free: panels s + 2, s + 3 go there (at s = 0 they were requested above)
    const int nreq = max(0, min(nsteps, s + 4) - requested);
    step(s, acc0, acc1, s > 0, nreq);
    step(s + 1, acc1, acc0, true, 0);
  }
  if (s < nsteps) {
    sync_pair(s, 1);
    step(s, acc0, acc1, s > 0, 0);
    // the last tile's squares, not hidden behind anything
    float ss = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) ss = fmaf(acc0[m][n][e], acc0[m][n][e], ss);
    finish_prev(acc0, ss, tj0 + nsteps - 1);
  } else {
    float ss = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) ss = fmaf(acc1[m][n][e], acc1[m][n][e], ss);
    finish_prev(acc1, ss, tj0 + nsteps - 1);
  }
  GPSTAMP(30);
  for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d, 64);
  if (lane == 0) s_part[wave] = (double)tot;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < GP_THREADS / 64; ++w) t += s_part[w];
    (branch ? part_y : part_x)[item] = t;
  }
}

// ---- Gram for deep contractions (batch > 128: BASELINE configs[3], global batch 1024), 256 x 256 tiles --------------
// Tile (ti, tj), ti <= tj, of branch b per workgroup on g2_product (vicreg_tiles.h); partial = sum of squares of its
// off-diagonal elements (x 2 above the diagonal).  Rows beyond D repeat row D - 1 on the way in and are masked in the
// epilogue.
__global__ __launch_bounds__(G2_THREADS, 2) void vicreg_gram256_kernel(const unsigned short* __restrict__ Xt_x,
                                                                       const unsigned short* __restrict__ Xt_y,
                                                                       double* __restrict__ part_x,
                                                                       double* __restrict__ part_y, int D, int Kpad,
                                                                       int ntile, int ntri) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_g2[];   // 2 buffers x (A 32 KB + B 32 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int r = lane & 15, q = lane >> 4;
  // XCD placement as in vicreg_gram_pair_kernel: an XCD's L2 serves one branch
  const int xslot = blockIdx.x & 7, branch = xslot >> 2;
  // Round 4: which tiles an XCD works on at the same time.  Workgroups go to the XCDs round-robin by block index; dealt
  // tile by tile along the rows of the triangle (rounds 2-3), the 32 tiles resident on an XCD were one row panel against
  // 32 column panels -- 33 panels of 512 KB through a 4 MB L2, 12.7 x the operands fetched from beyond it
  // (profiles/r03g_traffic.json).  Now an XCD takes CONTIGUOUS runs of 32 tiles of an enumeration that walks strips of
  // four tile rows column by column: its resident tiles are 4 row panels x 8 column panels (6 MB).
  const int q8 = blockIdx.x >> 3;                       // this XCD's q8-th workgroup
  const int item = (q8 >> 5) * 128 + (xslot & 3) * 32 + (q8 & 31);
  if (item >= ntri) return;
  int ti, tj;
  {
    int t = item, I = 0;
    for (;;) {                                          // strip I: tile rows 4 I .. 4 I + h - 1, columns 4 I .. ntile - 1
      const int h = min(4, ntile - 4 * I), w = ntile - 4 * I;
      const int cnt = h * w - h * (h - 1) / 2;          // the strip's tiles on or above the diagonal
      if (t < cnt) {
        // column-major inside the strip: column c (from the strip's first) has min(c + 1, h) tiles
        int c = 0;
        while (c < h - 1 && t >= c + 1) { t -= c + 1; ++c; }
        if (c == h - 1) { c += t / h; t -= (t / h) * h; }
        ti = 4 * I + t; tj = 4 * I + c;
        break;
      }
      t -= cnt; ++I;
    }
  }
  const unsigned short* Xt = branch ? Xt_y : Xt_x;
  vc_f32x4 acc[8][4];
  vc_zero(acc);
  g2_product(Xt, (unsigned)Kpad, D, ti * G2_T, Xt, (unsigned)Kpad, D, tj * G2_T, 0, Kpad / G2_BK, s_g2, acc);

  // ---- epilogue: C/D layout of a 16 x 16 tile: col = lane & 15, row = 4 (lane >> 4) + reg
  float ss = 0.f;
  const bool diag = ti == tj, ragged = (D % G2_T) != 0 && (tj == ntile - 1);
  if (diag || ragged) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = wr * 128 + 16 * m + 4 * q + e, col = wc * 64 + 16 * n + r;
          const bool ok = ti * G2_T + row < D && tj * G2_T + col < D && !(diag && row == col);
          const float v = acc[m][n][e];
          if (ok) ss = fmaf(v, v, ss);
        }
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = fmaf(acc[m][n][e], acc[m][n][e], ss);
  }
  for (int d = 32; d > 0; d >>= 1) ss += __shfl_xor(ss, d, 64);
  double* s_part = reinterpret_cast<double*>(s_g2);       // the staging buffers are idle now (barrier above)
  if (lane == 0) s_part[wave] = (double)ss;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int w = 0; w < G2_THREADS / 64; ++w) tot += s_part[w];
    (branch ? part_y : part_x)[item] = diag ? tot : 2.0 * tot;
  }
}

int vicreg_launch_feature_gram(const VicregWs& w, char* ws, int D, hipStream_t stream, bool launch) {
  const unsigned short* xt_x = (const unsigned short*)(ws + w.xt_x);
  const unsigned short* xt_y = (const unsigned short*)(ws + w.xt_y);
  double* gram_x = (double*)(ws + w.gram_x);
  double* gram_y = (double*)(ws + w.gram_y);
  if (w.Kpad == 128) {
    const int nitems = gp_nitems(w.ntile);   // pair kernel: one workgroup per (branch, row-panel pair, run of column panels)
    if (launch) {
      const size_t lds = (size_t)GP_RING * GP_PANEL_BYTES;
      (void)hipFuncSetAttribute((const void*)vicreg_gram_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(vicreg_gram_pair_kernel, dim3(8 * ((nitems + 3) / 4)), dim3(GP_THREADS), lds, stream, xt_x, xt_y,
                         gram_x, gram_y, D, w.ntile, nitems);
    }
    return nitems;
  }
  if (w.t256) {                              // deep contractions: 256 x 256 tiles
    const int nt256 = (D + G2_T - 1) / G2_T, ngram = nt256 * (nt256 + 1) / 2;
    if (launch) {
      const size_t lds = 2 * (size_t)G2_BUF_BYTES;
      (void)hipFuncSetAttribute((const void*)vicreg_gram256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      // (q8 = block >> 3 runs over 32 per 128 items: see the kernel's enumeration)
      hipLaunchKernelGGL(vicreg_gram256_kernel, dim3(8 * 32 * ((ngram + 127) / 128)), dim3(G2_THREADS), lds, stream, xt_x, xt_y,
                         gram_x, gram_y, D, w.Kpad, nt256, ngram);
    }
    return ngram;
  }
  if (launch)
    hipLaunchKernelGGL(vicreg_gram_kernel, dim3(w.ngram, 2), dim3(256), 0, stream, xt_x, xt_y, gram_x, gram_y, D, w.Kpad,
                       w.ntile);
  return w.ngram;
}
