// Sound matching (MI355X / gfx950): the per-sound losses of the matcher (inverse-audio-synthesis_amd/match.py), the L1 of
// two spectrogram tensors and the MR-STFT sums, a value per row.
//
// The reference's inverse loop -- params -> synth -> mel-L1 against the true audio -- is the commented-out block
// /root/reference/audio_to_params.py:56-172; its notebook wants one candidate and one distance per test sound
// (/root/reference/evaluate_audio_representations.py:202-231).  Fitting each sound on its own needs a loss per sound
// (a batch mean couples every sound's gradient to the batch size) and an optimizer whose state is per row.
//
// l1_rows_partials_kernel: grid (nchunks, B); workgroup (c, b) sums |v - t| over elements [c L1R_CHUNK, (c + 1) L1R_CHUNK)
//   of row b.  Thread t takes elements chunk + (k L1R_THREADS + t) * 4 + e, k < L1R_ITERS, e < 4, and adds them one by
//   one in that order whether it loads them as float4 or as floats (a row's 16-byte alignment depends on its position in
//   the batch when the row length is not a multiple of 4: the order of additions must not).  The 256 fp32 sums are
//   folded in fp64 in a fixed butterfly.  Nothing depends on b but the row pointer: a row's partials are the same bits
//   wherever it sits in the batch.
// l1_rows_fold_kernel: one lane per row adds the row's partials in chunk order and divides by the row length (fp64).
// mrstft_rows_partials_kernel / mrstft_rows_fold_kernel: the same two levels for the three sums of one resolution of the
//   MR-STFT loss, {sum (T - V)^2, sum T^2, sum |ln V - ln T|} per row, each element's terms formed as in the batch STFT
//   loss kernels (spectral_kernels.hip, LOSS2: fmaf for the squares, the difference of two __log2f, ln 2 applied to the
//   row's sum); the fold is a wave per row.  mrstft_rows_total_kernel / mrstft_coef_rows_kernel: mrstft_total_kernel /
//   mrstft_coef_kernel (spectral_grad_kernels.hip) once per row.
// The optimiser steps (match_adam_kernel, match_tied_kernel) are in match_step_kernels.hip.
#include "ias_common.h"
#include <cstdint>

#define L1R_THREADS 256
#define L1R_ITERS 4
#define L1R_CHUNK (L1R_THREADS * 4 * L1R_ITERS)      // 4096 floats per workgroup

__global__ __launch_bounds__(L1R_THREADS) void l1_rows_partials_kernel(const float* __restrict__ v,
                                                                       const float* __restrict__ t, long long n,
                                                                       int nchunks, double* __restrict__ partials) {
  __shared__ double s_red[L1R_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y;
  const float* vr = v + (size_t)b * n;
  const float* tr = t + (size_t)b * n;
  const long long base = (long long)c * L1R_CHUNK;
  const bool vec = ((reinterpret_cast<uintptr_t>(vr) | reinterpret_cast<uintptr_t>(tr)) & 15) == 0;
  float acc = 0.0f;
#pragma unroll
  for (int it = 0; it < L1R_ITERS; ++it) {
    const long long i = base + ((long long)it * L1R_THREADS + threadIdx.x) * 4;
    if (vec && i + 3 < n) {
      const float4 a = *reinterpret_cast<const float4*>(vr + i), q = *reinterpret_cast<const float4*>(tr + i);
      acc += fabsf(a.x - q.x);
      acc += fabsf(a.y - q.y);
      acc += fabsf(a.z - q.z);
      acc += fabsf(a.w - q.w);
    } else {
      for (int e = 0; e < 4; ++e)
        if (i + e < n) acc += fabsf(vr[i + e] - tr[i + e]);
    }
  }
  double s = (double)acc;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = s_red[0];
    for (int w = 1; w < L1R_THREADS / 64; ++w) r += s_red[w];
    partials[(size_t)b * nchunks + c] = r;
  }
}

__global__ __launch_bounds__(256) void l1_rows_fold_kernel(const double* __restrict__ partials, int B, int nchunks,
                                                          double count, float* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (size_t)b * nchunks;
  double s = p[0];
  for (int c = 1; c < nchunks; ++c) s += p[c];
  out[b] = (float)(s / count);
}

// ------------------------------------------------------------------------------------------------ per-row MR-STFT
// Thread t of workgroup (c, b) takes the same 16 elements as in l1_rows_partials_kernel, in the same order.  A chunk that
// ends at least 4 elements before the row's end is read with aligned float4 loads, all 8 issued before the arithmetic,
// whatever the row's 16-byte phase ph (both operands start on a 16-byte boundary, so their rows share ph): the thread's
// elements i .. i+3 are the last 4 - ph of the float4 it loads and the first ph of the next one, which lane + 1 loaded
// (lane 63 loads it itself).  Every other chunk element by element.  The V and T of the three auraloss resolutions at
// B = 128, 4 s @ 44.1 kHz are 2 x 1.24 GB: rows of 1471 x 513 and 3529 x 257 floats sit at every phase.
#define MRR_MAX_RES 8

__device__ __forceinline__ float4 shfl_down_f4(const float4& x) {
  return make_float4(__shfl_down(x.x, 1, 64), __shfl_down(x.y, 1, 64), __shfl_down(x.z, 1, 64), __shfl_down(x.w, 1, 64));
}

__global__ __launch_bounds__(L1R_THREADS) void mrstft_rows_partials_kernel(const float* __restrict__ v,
                                                                           const float* __restrict__ t, long long n,
                                                                           int nchunks, double* __restrict__ partials) {
  __shared__ double s_red[3][L1R_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y;
  const float* vr = v + (size_t)b * n;
  const float* tr = t + (size_t)b * n;
  const long long base = (long long)c * L1R_CHUNK;
  // the buffers (not the rows) start on a 16-byte boundary: an aligned float4 around a row's first element stays inside
  const bool vec = ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(t)) & 15) == 0;
  float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
  auto add = [&](float vv, float tt) {
    const float d = tt - vv;
    l0 = fmaf(d, d, l0);
    l1 = fmaf(tt, tt, l1);
    l2 += fabsf(__log2f(vv) - __log2f(tt));
  };
  if (vec && base + L1R_CHUNK + 4 <= n) {
    const int ph = (int)((reinterpret_cast<uintptr_t>(vr) >> 2) & 3);       // uniform over the workgroup
    const float4* va = reinterpret_cast<const float4*>(vr - ph);             // va[m]: row elements 4 m - ph .. 4 m - ph + 3
    const float4* ta = reinterpret_cast<const float4*>(tr - ph);
    float4 a[L1R_ITERS], q[L1R_ITERS];
#pragma unroll
    for (int it = 0; it < L1R_ITERS; ++it) {
      const long long m = (base >> 2) + (long long)it * L1R_THREADS + threadIdx.x;
      a[it] = va[m];
      q[it] = ta[m];
    }
    if (ph == 0) {
#pragma unroll
      for (int it = 0; it < L1R_ITERS; ++it) {
        add(a[it].x, q[it].x);
        add(a[it].y, q[it].y);
        add(a[it].z, q[it].z);
        add(a[it].w, q[it].w);
      }
    } else {
      float4 an[L1R_ITERS], qn[L1R_ITERS];
#pragma unroll
      for (int it = 0; it < L1R_ITERS; ++it) {
        an[it] = shfl_down_f4(a[it]);
        qn[it] = shfl_down_f4(q[it]);
      }
      if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int it = 0; it < L1R_ITERS; ++it) {
          const long long m = (base >> 2) + (long long)it * L1R_THREADS + threadIdx.x + 1;
          an[it] = va[m];
          qn[it] = ta[m];
        }
      }
#pragma unroll
      for (int it = 0; it < L1R_ITERS; ++it) {
        if (ph == 1) {
          add(a[it].y, q[it].y); add(a[it].z, q[it].z); add(a[it].w, q[it].w); add(an[it].x, qn[it].x);
        } else if (ph == 2) {
          add(a[it].z, q[it].z); add(a[it].w, q[it].w); add(an[it].x, qn[it].x); add(an[it].y, qn[it].y);
        } else {
          add(a[it].w, q[it].w); add(an[it].x, qn[it].x); add(an[it].y, qn[it].y); add(an[it].z, qn[it].z);
        }
      }
    }
  } else {
    for (int it = 0; it < L1R_ITERS; ++it) {
      const long long i = base + ((long long)it * L1R_THREADS + threadIdx.x) * 4;
      for (int e = 0; e < 4; ++e)
        if (i + e < n) add(vr[i + e], tr[i + e]);
    }
  }
  double s0 = (double)l0, s1 = (double)l1, s2 = (double)l2;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s0 += __shfl_xor(s0, d, 64);
    s1 += __shfl_xor(s1, d, 64);
    s2 += __shfl_xor(s2, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_red[0][threadIdx.x >> 6] = s0;
    s_red[1][threadIdx.x >> 6] = s1;
    s_red[2][threadIdx.x >> 6] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double r = s_red[threadIdx.x][0];
    for (int w = 1; w < L1R_THREADS / 64; ++w) r += s_red[threadIdx.x][w];
    partials[((size_t)b * nchunks + c) * 3 + threadIdx.x] = r;
  }
}

// One wave per row: the row's partials pass through LDS in tiles of MRR_FOLD_TILE chunks (coalesced loads), and lane k < 3
// adds column k in chunk order.  (One lane per row, reading its partials straight from memory, took ~100 us for rows of
// ~200 chunks at B = 128.)
#define MRR_FOLD_TILE 512

__global__ __launch_bounds__(64) void mrstft_rows_fold_kernel(const double* __restrict__ partials, int nchunks,
                                                             double* __restrict__ sums) {
  __shared__ double s_p[3 * MRR_FOLD_TILE];
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* p = partials + (size_t)b * nchunks * 3;
  double acc = 0.0;
  for (int c0 = 0; c0 < nchunks; c0 += MRR_FOLD_TILE) {
    const int nc = min(MRR_FOLD_TILE, nchunks - c0);
    for (int i = lane; i < 3 * nc; i += 64) s_p[i] = p[3 * (size_t)c0 + i];
    __syncthreads();
    if (lane < 3) {
      int c = 0;
      if (c0 == 0) { acc = s_p[lane]; c = 1; }
      for (; c < nc; ++c) acc += s_p[3 * c + lane];
    }
    __syncthreads();
  }
  if (lane < 3) sums[3 * (size_t)b + lane] = lane == 2 ? acc * 0.6931471805599453 : acc;   // log terms were taken in log2
}

struct MrRowsTotalArgs { const double* sums[MRR_MAX_RES]; double count[MRR_MAX_RES]; int nres; };

// out[b] = (sum_k sqrt(s_k[b][0]) / sqrt(s_k[b][1]) + s_k[b][2] / count_k) / nres: mrstft_total_kernel's expression and
// order for each row
__global__ __launch_bounds__(256) void mrstft_rows_total_kernel(const MrRowsTotalArgs a, int B, float* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double total = 0.0;
  for (int k = 0; k < a.nres; ++k) {
    const double* s = a.sums[k] + 3 * (size_t)b;
    const double term = sqrt(s[0]) / sqrt(s[1]) + s[2] / a.count[k];
    total = k == 0 ? term : total + term;
  }
  out[b] = (float)(total / (double)a.nres);
}

// mrstft_coef_kernel's pair for each row with its own cotangent g_rows[b]; {0, 0} where g_rows[b] == 0
__global__ __launch_bounds__(256) void mrstft_coef_rows_kernel(const double* __restrict__ s, const float* __restrict__ g_rows,
                                                              double count, int nres, int B, double* __restrict__ coef) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double g = (double)g_rows[b];
  if (g == 0.0) {
    coef[2 * (size_t)b] = 0.0;
    coef[2 * (size_t)b + 1] = 0.0;
    return;
  }
  const double den = sqrt(s[3 * (size_t)b]) * sqrt(s[3 * (size_t)b + 1]);
  coef[2 * (size_t)b] = den > 0.0 ? g / ((double)nres * den) : 0.0;
  coef[2 * (size_t)b + 1] = g / ((double)nres * count);
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ias_l1_rows_partials_count(long long n) {
  if (n <= 0 || (n + L1R_CHUNK - 1) / L1R_CHUNK > 2147483647LL) return IAS_ERR_ARG;
  return (int)((n + L1R_CHUNK - 1) / L1R_CHUNK);
}

extern "C" int ias_l1_rows(const float* values, const float* target, int B, long long n, double* partials, float* out,
                           void* stream_) {
  if (!values || !target || !partials || !out || B <= 0 || B > 65535 || n <= 0) return IAS_ERR_ARG;
  const int nchunks = ias_l1_rows_partials_count(n);
  if (nchunks <= 0) return IAS_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(l1_rows_partials_kernel, dim3(nchunks, B), dim3(L1R_THREADS), 0, stream, values, target, n, nchunks,
                     partials);
  hipLaunchKernelGGL(l1_rows_fold_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, partials, B, nchunks, (double)n, out);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_mrstft_rows_partials_count(long long n) { return ias_l1_rows_partials_count(n); }

extern "C" int ias_mrstft_rows(const float* values, const float* target, int B, long long n, double* partials, double* sums,
                               void* stream_) {
  if (!values || !target || !partials || !sums || B <= 0 || B > 65535 || n <= 0) return IAS_ERR_ARG;
  const int nchunks = ias_l1_rows_partials_count(n);
  if (nchunks <= 0) return IAS_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(mrstft_rows_partials_kernel, dim3(nchunks, B), dim3(L1R_THREADS), 0, stream, values, target, n,
                     nchunks, partials);
  hipLaunchKernelGGL(mrstft_rows_fold_kernel, dim3(B), dim3(64), 0, stream, partials, nchunks, sums);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_mrstft_rows_total(const double* const* sums_host, const double* counts_host, int nres, int B, float* out,
                                     void* stream_) {
  if (!sums_host || !counts_host || !out || nres < 1 || nres > MRR_MAX_RES || B <= 0) return IAS_ERR_ARG;
  MrRowsTotalArgs a;
  for (int k = 0; k < MRR_MAX_RES; ++k) { a.sums[k] = nullptr; a.count[k] = 1.0; }
  for (int k = 0; k < nres; ++k) {
    if (!sums_host[k] || !(counts_host[k] > 0.0)) return IAS_ERR_ARG;
    a.sums[k] = sums_host[k]; a.count[k] = counts_host[k];
  }
  a.nres = nres;
  hipLaunchKernelGGL(mrstft_rows_total_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream_, a, B, out);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_mrstft_coef_rows(const double* sums, const float* g_rows, double count, int nres, int B, double* coef,
                                    void* stream_) {
  if (!sums || !g_rows || !coef || nres < 1 || nres > MRR_MAX_RES || B <= 0 || !(count > 0.0)) return IAS_ERR_ARG;
  hipLaunchKernelGGL(mrstft_coef_rows_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream_, sums, g_rows, count,
                     nres, B, coef);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
