// What the STFT forward (spectral_kernels.hip) and the table-driven frame gradient (stft_frame_grad_kernels.hip) share:
// packed complex arithmetic, the small DFTs, wave-level exchanges, the frame loads and the exchange-scratch layout.
#pragma once
#include "ias_common.h"

// Complex numbers as 2-wide vectors: complex add/sub are one packed op (a packed fp32 op costs the SIMD 4 clocks, two
// plain ones 2 + 2: the same arithmetic time, fewer instructions to issue).  8-byte aligned: LDS accesses are ds_*_b64.
typedef float cpx __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// floats of the re-packed mel weight table in LDS (every filter padded to a multiple of four taps), rounded to 16 bytes
__host__ __device__ static inline int mel_padded_words(int mel_nnz, int n_out) {
  return n_out > 0 ? ((mel_nnz + 3 * n_out + 3) & ~3) : 0;
}
__device__ __forceinline__ cpx cmk(float x, float y) { return (cpx){x, y}; }
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { return a + b; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { return a - b; }
// Operations with a swapped or negated operand -- a complex multiply, a multiplication by -i.  Written as 2-wide vector
// expressions (the IAS_DIAG forms below, the superseded code) their operand (-a.y, a.y) or (a.y, -a.x) is BUILT first, a
// v_xor_b32 for the sign and a v_mov_b32 for the pair (4 + 2 clocks) in front of every use: the compiler does not fold
// the swap and the sign into the packed instruction's op_sel / neg modifiers (31 + 41 such instructions in the 343 of
// the n_fft 1024 kernel's frame block).  So
//   cmul        is written per component: a plain fp32 instruction takes its sign as a source modifier and either half
//               of a pair as its operand, and four of them cost the SIMD what pk_mul + pk_fma do (4 x 2 = 2 x 4 clocks);
//   a + (-i) x  and its kin are ONE v_pk_add_f32 whose modifiers carry the swap and the sign (inline asm: written per
//               component the compiler re-packs them and pays for the sign with extra subtractions); a multiplication
//               by -i is never materialised, the add that consumes it takes it.
// Every product, every fused multiply-add and every rounding point is the vector form's -- the asm adds take sums,
// never a product the compiler would have contracted into them -- so the results are the same bits
// (tests/test_fft_forms_gpu.py: every kernel built on these helpers, product library against diagnostic library).
#ifdef IAS_DIAG
__device__ __forceinline__ cpx cmul(cpx a, cpx b) {
  return __builtin_elementwise_fma((cpx){-a.y, a.y}, (cpx){b.y, b.x}, (cpx){a.x, a.x} * b);
}
__device__ __forceinline__ cpx cmul_negi(cpx a) { return (cpx){a.y, -a.x}; }  // a * (-i)
__device__ __forceinline__ cpx cadd_negi(cpx a, cpx x) { return a + cmul_negi(x); }   // a + (-i) x
__device__ __forceinline__ cpx csub_negi(cpx a, cpx x) { return a - cmul_negi(x); }   // a - (-i) x
__device__ __forceinline__ cpx cnegi_sub(cpx x, cpx a) { return cmul_negi(x) - a; }   // (-i) x - a
#else
__device__ __forceinline__ cpx cmul(cpx a, cpx b) {
  return cmk(__builtin_fmaf(-a.y, b.y, a.x * b.x), __builtin_fmaf(a.y, b.x, a.x * b.y));
}
__device__ __forceinline__ cpx cadd_negi(cpx a, cpx x) {    // a + (-i) x = (a.x + x.y, a.y - x.x)
  cpx r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(x)); return r;
}
__device__ __forceinline__ cpx csub_negi(cpx a, cpx x) {    // a - (-i) x = (a.x - x.y, a.y + x.x)
  cpx r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(x)); return r;
}
__device__ __forceinline__ cpx cnegi_sub(cpx x, cpx a) {    // (-i) x - a = (x.y - a.x, -x.x - a.y)
  cpx r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[1,1]" : "=v"(r) : "v"(x), "v"(a)); return r;
}
#endif

// a * (1, -0): W^0 as the twiddle tables hold it (cos 0, -sin 0), without reading it.  cmul's own two results for that
// operand -- a.x * 1 is a.x, and (-a.y)(-0) = a.y * 0, a.x * (-0) = (-a.x) * 0 with their signs -- so the same bits, zeros
// included; the zero is an inline constant and the signs are source modifiers: two instructions, no register.
__device__ __forceinline__ cpx cmul_unit(cpx a) { return cmk(__builtin_fmaf(a.y, 0.0f, a.x), __builtin_fmaf(-a.x, 0.0f, a.y)); }

// forward DFTs (kernel e^{-2 pi i nk/R}), in place, natural order.  A multiplication by -i is never materialised: the
// add or subtract that consumes it takes the swap and the sign.
__device__ __forceinline__ void dft4(cpx& v0, cpx& v1, cpx& v2, cpx& v3) {
  const cpx t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3), t3 = csub(v1, v3);
  v0 = cadd(t0, t2); v1 = cadd_negi(t1, t3); v2 = csub(t0, t2); v3 = csub_negi(t1, t3);
}
__device__ __forceinline__ void dft8(cpx* v) {
  cpx e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
  cpx o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
  dft4(e0, e1, e2, e3);
  dft4(o0, o1, o2, o3);
  const float h = 0.70710678118654752f;
  o1 = cadd_negi(o1, o1) * h;                         // * W8^1 = (1 - i)/sqrt2
  o3 = cnegi_sub(o3, o3) * h;                         // * W8^3 = (-1 - i)/sqrt2
  v[0] = cadd(e0, o0); v[4] = csub(e0, o0);
  v[1] = cadd(e1, o1); v[5] = csub(e1, o1);
  v[2] = cadd_negi(e2, o2); v[6] = csub_negi(e2, o2); // * W8^2 = -i
  v[3] = cadd(e3, o3); v[7] = csub(e3, o3);
}
__device__ __forceinline__ void dft16(cpx* v) {
  cpx e[8], o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { e[i] = v[2 * i]; o[i] = v[2 * i + 1]; }
  dft8(e);
  dft8(o);
  // W16^k, k = 0..7
  const float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f, h = 0.70710678118654752f;
  const cpx w[8] = {cmk(1.f, 0.f), cmk(c1, -s1), cmk(h, -h), cmk(s1, -c1),
                    cmk(0.f, -1.f), cmk(-s1, -c1), cmk(-h, -h), cmk(-c1, -s1)};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const cpx t = cmul(o[k], w[k]);
    v[k] = cadd(e[k], t);
    v[k + 8] = csub(e[k], t);
  }
}
template <int R> __device__ __forceinline__ void dftR(cpx* v);
template <> __device__ __forceinline__ void dftR<4>(cpx* v) { dft4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ void dftR<8>(cpx* v) { dft8(v); }
template <> __device__ __forceinline__ void dftR<16>(cpx* v) { dft16(v); }

__device__ __forceinline__ int reflect_index(int i, int T) {
  if (i < 0) i = -i;
  if (i >= T) i = 2 * (T - 1) - i;
  return i;
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// LDS traffic inside one wave only needs ORDERING, not a workgroup barrier and not a wait: the waves of a workgroup
// work on different frames with private scratch, and the LDS instructions of one wave execute in program order
// (LLVM's AMDGPU memory model puts no s_waitcnt on a wavefront-scope fence for that reason).  So a hand-over between
// lanes of the wave is a compiler-level fence; the s_waitcnt lgkmcnt(0) that used to sit here drained the wave's LDS
// queue eight times per frame.  The compiler still waits, with exact counts, where a loaded VALUE is consumed.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- register <-> lane-bits transpose (round 4): the first exchange of the radix-8 kernels without LDS.
// Pass 1 leaves element (k1, a, c) in register k1 of lane 8 a + c; pass 2 wants it in register a of lane 8 k1 + c: an
// 8 x 8 transpose between the register index and lane bits 3..5.  Bit by bit: register bit 0 <-> lane bit 3 (distance 8
// inside a row of 16: two bank-masked DPP row rotations and a copy per register pair), bit 1 <-> lane bit 4
// (v_permlane16_swap: rows 1, 3 of one register against rows 0, 2 of the other), bit 2 <-> lane bit 5
// (v_permlane32_swap).  32 + 8 + 8 = 48 VALU instructions for the 8 complex values of a lane, against 8 ds_write_b64
// (6 LDS cycles each) + 8 ds_read_b64 and two LDS round trips of latency (checked lane by lane against the LDS transpose:
// scripts/diag/permlane_swap.hip).  The second exchange transposes the register index with lane bits 0..2, for which
// gfx950 has no swap instruction (three DPP instructions per pair and level: 72): it stays in LDS.
typedef unsigned x_u2 __attribute__((ext_vector_type(2)));
template <int L> __device__ __forceinline__ void xchg_pair(float& f0, float& f1) {
  unsigned r0 = __float_as_uint(f0), r1 = __float_as_uint(f1);
  if (L == 5) { const x_u2 t = __builtin_amdgcn_permlane32_swap(r0, r1, false, false); r0 = t.x; r1 = t.y; }
  else if (L == 4) { const x_u2 t = __builtin_amdgcn_permlane16_swap(r0, r1, false, false); r0 = t.x; r1 = t.y; }
  else {
    // lanes with bit 3 set (banks 2, 3 of a row of 16): r0 <- r1 of lane ^ 8; lanes with bit 3 clear: r1 <- r0 of lane ^ 8
    const unsigned old0 = r0;
    r0 = __builtin_amdgcn_update_dpp(r0, r1, 0x128 /* row_ror:8 */, 0xf, 0xc, false);
    r1 = __builtin_amdgcn_update_dpp(r1, old0, 0x128, 0xf, 0x3, false);
  }
  f0 = __uint_as_float(r0); f1 = __uint_as_float(r1);
}
// u[k1] of lane (a, c)  ->  u[a] of lane (k1, c)
__device__ __forceinline__ void xchg_reg_lane345(cpx (&u)[8]) {
#pragma unroll
  for (int comp = 0; comp < 2; ++comp) {
    float f[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) f[q] = comp ? u[q].y : u[q].x;
    xchg_pair<3>(f[0], f[1]); xchg_pair<3>(f[2], f[3]); xchg_pair<3>(f[4], f[5]); xchg_pair<3>(f[6], f[7]);
    xchg_pair<4>(f[0], f[2]); xchg_pair<4>(f[1], f[3]); xchg_pair<4>(f[4], f[6]); xchg_pair<4>(f[5], f[7]);
    xchg_pair<5>(f[0], f[4]); xchg_pair<5>(f[1], f[5]); xchg_pair<5>(f[2], f[6]); xchg_pair<5>(f[3], f[7]);
#pragma unroll
    for (int q = 0; q < 8; ++q) { if (comp) u[q].y = f[q]; else u[q].x = f[q]; }
  }
}

// Loads the 2R samples of frame f that lane `lane` owns in pass 1 (points 64*n1 + lane, n1 < R).
// Interior frames on 8-byte-aligned rows: R coalesced 8-byte loads (512 B per wave instruction);
// frames that touch the row ends (reflect padding) or odd alignments: per-sample indexing.
template <int R, int N2>
__device__ __forceinline__ void load_frame(const float* __restrict__ arow, int T, int hop, int f, int lane,
                                           float (&x)[2 * R]) {
  const int g0 = f * hop - N2;
  if (g0 >= 0 && g0 + 2 * N2 <= T && (((g0 | T) & 1) == 0)) {
    // interior frame: R 8-byte loads off ONE address register pair (immediate offsets 512 n1).  The pointer is made
    // opaque and the edge path's values pass through empty asm statements: left alone, the compiler sinks the loads of
    // both paths into one block of 2 R single-dword loads from 2 R separate 64-bit addresses (32 address VGPRs, twice
    // the memory instructions) -- for every frame, to share code with the two edge frames per row.
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) f32x2_t* glb_f2p;    // stays a GLOBAL pointer through the asm
    glb_f2p p = (glb_f2p)(reinterpret_cast<const f32x2_t*>(arow + g0) + lane);
    asm volatile("" : "+v"(p));
#pragma unroll
    for (int n1 = 0; n1 < R; ++n1) { const f32x2_t q = p[64 * n1]; x[2 * n1] = q[0]; x[2 * n1 + 1] = q[1]; }
  } else {
#pragma unroll
    for (int n1 = 0; n1 < R; ++n1) {
      const int m = g0 + 2 * (64 * n1 + lane);
      x[2 * n1] = arow[reflect_index(m, T)];
      x[2 * n1 + 1] = arow[reflect_index(m + 1, T)];
      asm volatile("" : "+v"(x[2 * n1]), "+v"(x[2 * n1 + 1]));
    }
  }
}

// Exchange scratch of the radix-8 kernels: 64 rows of IAS_S2_ROW complex values per wave, element (row, col) at IAS_S2_AT.
// The LDS rules of MI355X_MICROARCH.md (ds_write_b64: 4 x 16 contiguous lanes over 32 dword banks; ds_read_b64: 2 x 32
// lanes over 64; ds_read_b128: 4 x 16 lanes) reproduce the counter exactly (scripts/diag/lds_exchange_model.py):
//   rows of 9 (the usual odd padding): the pass-1 scatter [(q 8 + c)][a] has 16 lanes at 9 c + a (c < 8, a in {2j, 2j+1}),
//     and 9 * 7 + 1 = 64 wraps onto 0: 2-way in every group of those eight stores (32 cycles per frame); the upper-half
//     stores of the unpack (index i + i / 8) wrap the same way (16) and its mirrored reads cost 8: 56 measured
//     (profiles/r03f_pmc_stft.txt, the kernel without the mel part);
//   rows of 10, two pad elements per eight in the upper half: the pass-1 scatter and the upper-half stores are clean, the
//     row reads become 16-byte reads (conflict-free in their lane groups, half the instructions), but the pass-2 scatter
//     [(k1 8 + d)][dd] now has its two k1 of a group 80 elements = 0 (mod 16) apart: 32 + 8 = 40 measured.
// The three patterns cannot all be conflict-free in this family (rows of 8 ... 18 elements with an offset per 8 rows,
// searched exhaustively: the 2-way conflict moves between the two scatters and the row reads), and a conflict in a STORE is
// the cheap place for it (6 issue cycles cover 4 of its 8 array cycles; a read pays all of them).  Rows of 10: 15 % fewer
// LDS cycles per frame than rows of 9, the 1024-point forward 53 -> 50.4 us.
// 640 complex values per wave also hold the mel projection's segment-major power rows at a stride of 72 floats (its scatter's
// ds_write_b32: 43 conflict cycles per frame at a stride of 65, 29 at 67, 22 at 74, 18 at 72 -- of which 2 cost time: a 2-way
// conflict of a 4-byte store hides behind its issue cycles; same model, same agreement with the counter).
#define IAS_S2_ROW 10
#define IAS_S2_AT(row, col) ((row) * IAS_S2_ROW + (col))
#define IAS_S2_UP(i) ((i) + (IAS_S2_ROW - 8) * ((i) >> 3))

// NSUB = 2: n_fft 2048 on the same 8-points-per-lane core.  The 1024 packed complex points split into their even and
// odd halves (decimation in time), each a 512-point transform through the three radix-8 passes above, one after the
// other through the same scratch; Z[k] = E[k] + W_1024^k O[k] and Z[k + 512] = E[k] - W_1024^k O[k] are combined in
// the lane that holds both (same k), which is also exactly the lower / upper split the half-spectrum unpack wants.
// The round-2 kernel transforms such a frame with a radix-16 first pass at 16 points per lane: 164 VGPRs, 9.2 KB of
// scratch per wave, 2-3 waves per SIMD and 7x the time of a 1024-point frame; this form costs 2.3x.
template <int NSUB> __device__ __forceinline__ void stft2_load_frame(const float* __restrict__ arow, int T, int hop, int f,
                                                                      int lane, float (&x)[16 * NSUB]) {
  if (NSUB == 1) {
    float (&x1)[16] = reinterpret_cast<float (&)[16]>(x);
    load_frame<8, 512>(arow, T, hop, f, lane, x1);
  } else {
    // lane, n1: samples 256 n1 + 4 lane .. + 3 = (even point, odd point) of the two half-transforms; x[16 sub + 2 n1 + c]
    const int g0 = f * hop - 1024;
    if (g0 >= 0 && g0 + 2048 <= T && ((reinterpret_cast<uintptr_t>(arow + g0) & 15) == 0)) {
      // (no opaque pointer here, unlike load_frame: measured slower for the 2048-point kernels, 145 vs 123 us forward)
      const f32x4* p = reinterpret_cast<const f32x4*>(arow + g0) + lane;
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) {
        const f32x4 q = p[64 * n1];
        x[2 * n1] = q[0]; x[2 * n1 + 1] = q[1]; x[16 + 2 * n1] = q[2]; x[16 + 2 * n1 + 1] = q[3];
      }
    } else {
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          x[16 * (c >> 1) + 2 * n1 + (c & 1)] = arow[reflect_index(g0 + 256 * n1 + 4 * lane + c, T)];
        }
    }
  }
}
