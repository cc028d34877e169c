// Output gain of sound matching (MI355X / gfx950): the per-sound level beside the 78 Voice parameters
// (inverse-audio-synthesis_amd/match.py: apply_gain, solve_gain).  The contract is include/ias_hip_gain.h.
//
// Three bandwidth-bound passes over [B, T] fp32 rows, grid (chunks, B), 256 threads, IAS_GAIN_CHUNK samples per workgroup:
//   gain_apply_kernel            out = a_b audio
//   gain_backward_kernel         g_audio = a_b g_out, and the chunk's partial of D_b = sum g_out audio (fp64)
//   gain_energy_kernel           the chunk's partials of sum target^2 and sum render^2 (fp64)
// and two folds with one lane per row, gain_backward_fold_kernel and gain_solve_fold_kernel, which add a row's partials
// in chunk order.  Thread t takes samples chunk + (k 256 + t) 4 + e, k < GAIN_ITERS, e < 4, as in l1_rows_partials_kernel
// (match_kernels.hip): as a float4 where the rows start on a 16-byte boundary and the four samples are inside the row,
// one by one otherwise, in the same order of additions.  A sample past the row's end is a zero term, which leaves an
// fp64 sum as it is.  All of a thread's loads are issued before the scale is computed: a_b costs one fp64 exp10 per
// thread, the same instructions whether one lane or all 64 of a wave run them, next to 32 samples per thread.
#include "ias_common.h"
#include <cstdint>

#define GAIN_THREADS 256
#define GAIN_ITERS (IAS_GAIN_CHUNK / (GAIN_THREADS * 4))
static_assert(GAIN_ITERS * GAIN_THREADS * 4 == IAS_GAIN_CHUNK, "a chunk is a whole number of float4 per thread");

// A_b of the gain law, fp64
__device__ __forceinline__ double gain_amplitude(float g01) {
  const double db = IAS_GAIN_DB_LO + (IAS_GAIN_DB_HI - IAS_GAIN_DB_LO) * (double)g01;
  return exp10(db / 20.0);
}

__device__ __forceinline__ float4 gain_load4(const float* __restrict__ row, long long i, long long T, bool vec) {
  if (vec && i + 3 < T) return *reinterpret_cast<const float4*>(row + i);
  float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i < T) x.x = row[i];
  if (i + 1 < T) x.y = row[i + 1];
  if (i + 2 < T) x.z = row[i + 2];
  if (i + 3 < T) x.w = row[i + 3];
  return x;
}

__device__ __forceinline__ void gain_store4(float* __restrict__ row, long long i, long long T, bool vec, const float4& x) {
  if (vec && i + 3 < T) {
    *reinterpret_cast<float4*>(row + i) = x;
    return;
  }
  if (i < T) row[i] = x.x;
  if (i + 1 < T) row[i + 1] = x.y;
  if (i + 2 < T) row[i + 2] = x.z;
  if (i + 3 < T) row[i + 3] = x.w;
}

__device__ __forceinline__ bool gain_aligned(const void* p, const void* q, const void* r = nullptr) {
  return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(r)) & 15) == 0;
}

// The 256 fp64 sums of a workgroup -> one value in thread 0: a fixed butterfly per wave, the waves in wave order.
__device__ __forceinline__ double gain_block_sum(double s, double* s_red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  double r = s_red[0];
  for (int w = 1; w < GAIN_THREADS / 64; ++w) r += s_red[w];
  return r;
}

__global__ __launch_bounds__(GAIN_THREADS) void gain_apply_kernel(const float* __restrict__ audio,
                                                                  const float* __restrict__ g01,
                                                                  float* __restrict__ out, long long T) {
  const int c = blockIdx.x, b = blockIdx.y;
  const float* xr = audio + (size_t)b * T;
  float* yr = out + (size_t)b * T;
  const long long base = (long long)c * IAS_GAIN_CHUNK + (long long)threadIdx.x * 4;
  const bool vec = gain_aligned(xr, yr);
  float4 x[GAIN_ITERS];
#pragma unroll
  for (int it = 0; it < GAIN_ITERS; ++it) x[it] = gain_load4(xr, base + (long long)it * GAIN_THREADS * 4, T, vec);
  const float a = (float)gain_amplitude(g01[b]);
#pragma unroll
  for (int it = 0; it < GAIN_ITERS; ++it)
    gain_store4(yr, base + (long long)it * GAIN_THREADS * 4, T, vec,
                make_float4(a * x[it].x, a * x[it].y, a * x[it].z, a * x[it].w));
}

__global__ __launch_bounds__(GAIN_THREADS) void gain_backward_kernel(const float* __restrict__ g_out,
                                                                     const float* __restrict__ audio,
                                                                     const float* __restrict__ g01,
                                                                     float* __restrict__ g_audio, long long T, int nchunks,
                                                                     double* __restrict__ partials) {
  __shared__ double s_red[GAIN_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y;
  const float* gr = g_out + (size_t)b * T;
  const float* xr = audio + (size_t)b * T;
  float* yr = g_audio + (size_t)b * T;
  const long long base = (long long)c * IAS_GAIN_CHUNK + (long long)threadIdx.x * 4;
  const bool vec = gain_aligned(gr, xr, yr);
  float4 g[GAIN_ITERS], x[GAIN_ITERS];
#pragma unroll
  for (int it = 0; it < GAIN_ITERS; ++it) {
    g[it] = gain_load4(gr, base + (long long)it * GAIN_THREADS * 4, T, vec);
    x[it] = gain_load4(xr, base + (long long)it * GAIN_THREADS * 4, T, vec);
  }
  const float a = (float)gain_amplitude(g01[b]);
  double acc = 0.0;
#pragma unroll
  for (int it = 0; it < GAIN_ITERS; ++it) {
    acc = fma((double)g[it].x, (double)x[it].x, acc);      // the product is exact in fp64: one rounding per addition
    acc = fma((double)g[it].y, (double)x[it].y, acc);
    acc = fma((double)g[it].z, (double)x[it].z, acc);
    acc = fma((double)g[it].w, (double)x[it].w, acc);
    gain_store4(yr, base + (long long)it * GAIN_THREADS * 4, T, vec,
                make_float4(a * g[it].x, a * g[it].y, a * g[it].z, a * g[it].w));
  }
  const double r = gain_block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[(size_t)b * nchunks + c] = r;
}

__global__ __launch_bounds__(256) void gain_backward_fold_kernel(const double* __restrict__ partials,
                                                                const float* __restrict__ g01, int B, int nchunks,
                                                                float* __restrict__ g_gain01) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (size_t)b * nchunks;
  double d = p[0];
  for (int c = 1; c < nchunks; ++c) d += p[c];
  const double k = (2.302585092994045684 / 20.0) * (IAS_GAIN_DB_HI - IAS_GAIN_DB_LO);      // d db / d g01 times ln 10 / 20
  g_gain01[b] = (float)(d * gain_amplitude(g01[b]) * k);
}

__global__ __launch_bounds__(GAIN_THREADS) void gain_energy_kernel(const float* __restrict__ target,
                                                                   const float* __restrict__ render, long long T,
                                                                   int nchunks, double* __restrict__ partials) {
  __shared__ double s_red[2][GAIN_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y;
  const float* tr = target + (size_t)b * T;
  const float* rr = render + (size_t)b * T;
  const long long base = (long long)c * IAS_GAIN_CHUNK + (long long)threadIdx.x * 4;
  const bool vec = gain_aligned(tr, rr);
  float4 t[GAIN_ITERS], r[GAIN_ITERS];
#pragma unroll
  for (int it = 0; it < GAIN_ITERS; ++it) {
    t[it] = gain_load4(tr, base + (long long)it * GAIN_THREADS * 4, T, vec);
    r[it] = gain_load4(rr, base + (long long)it * GAIN_THREADS * 4, T, vec);
  }
  double et = 0.0, er = 0.0;
#pragma unroll
  for (int it = 0; it < GAIN_ITERS; ++it) {
    et = fma((double)t[it].x, (double)t[it].x, et);
    et = fma((double)t[it].y, (double)t[it].y, et);
    et = fma((double)t[it].z, (double)t[it].z, et);
    et = fma((double)t[it].w, (double)t[it].w, et);
    er = fma((double)r[it].x, (double)r[it].x, er);
    er = fma((double)r[it].y, (double)r[it].y, er);
    er = fma((double)r[it].z, (double)r[it].z, er);
    er = fma((double)r[it].w, (double)r[it].w, er);
  }
  const double st = gain_block_sum(et, s_red[0]);
  const double sr = gain_block_sum(er, s_red[1]);
  if (threadIdx.x == 0) {
    partials[((size_t)b * nchunks + c) * 2] = st;
    partials[((size_t)b * nchunks + c) * 2 + 1] = sr;
  }
}

__global__ __launch_bounds__(256) void gain_solve_fold_kernel(const double* __restrict__ partials, int B, int nchunks,
                                                             float* __restrict__ g01) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (size_t)b * nchunks * 2;
  double et = p[0], er = p[1];
  for (int c = 1; c < nchunks; ++c) {
    et += p[2 * c];
    er += p[2 * c + 1];
  }
  float g = 0.75f;                                     // 0 dB
  if (isfinite(et) && isfinite(er) && et > 0.0 && er > 0.0) {
    const double db = fmin(fmax(10.0 * log10(et / er), IAS_GAIN_DB_LO), IAS_GAIN_DB_HI);
    g = (float)((db - IAS_GAIN_DB_LO) / (IAS_GAIN_DB_HI - IAS_GAIN_DB_LO));
  }
  g01[b] = g;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ias_gain_partials_count(long long T) {
  if (T <= 0 || (T + IAS_GAIN_CHUNK - 1) / IAS_GAIN_CHUNK > 2147483647LL) return IAS_ERR_ARG;
  return (int)((T + IAS_GAIN_CHUNK - 1) / IAS_GAIN_CHUNK);
}

// do two arrays of B T floats share a byte?
static bool gain_overlap(const float* p, const float* q, int B, long long T) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)T * sizeof(float);
  return a < b + bytes && b < a + bytes;
}

// IAS_OK and the chunk count of a row, or the refusal of B and T
static int gain_shape(int B, long long T, int* nchunks) {
  if (B < 1 || T < 1) return IAS_ERR_ARG;
  if (B > 65535 || (T + IAS_GAIN_CHUNK - 1) / IAS_GAIN_CHUNK > 2147483647LL) return IAS_ERR_UNSUPPORTED;
  *nchunks = ias_gain_partials_count(T);
  return IAS_OK;
}

extern "C" int ias_gain_apply(const float* audio, const float* g01, float* out, int B, long long T, void* stream_) {
  if (!audio || !g01 || !out) return IAS_ERR_ARG;
  int nchunks = 0;
  const int st = gain_shape(B, T, &nchunks);
  if (st != IAS_OK) return st;
  if (gain_overlap(audio, out, B, T)) return IAS_ERR_ARG;
  hipLaunchKernelGGL(gain_apply_kernel, dim3(nchunks, B), dim3(GAIN_THREADS), 0, (hipStream_t)stream_, audio, g01, out, T);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_gain_backward(const float* g_out, const float* audio, const float* g01, float* g_audio, float* g_gain01,
                                 double* partials, int B, long long T, void* stream_) {
  if (!g_out || !audio || !g01 || !g_audio || !g_gain01 || !partials) return IAS_ERR_ARG;
  int nchunks = 0;
  const int st = gain_shape(B, T, &nchunks);
  if (st != IAS_OK) return st;
  if (gain_overlap(g_out, g_audio, B, T) || gain_overlap(audio, g_audio, B, T)) return IAS_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(gain_backward_kernel, dim3(nchunks, B), dim3(GAIN_THREADS), 0, stream, g_out, audio, g01, g_audio, T,
                     nchunks, partials);
  hipLaunchKernelGGL(gain_backward_fold_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, partials, g01, B, nchunks,
                     g_gain01);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_gain_solve(const float* target, const float* render, float* g01, double* partials, int B, long long T,
                              void* stream_) {
  if (!target || !render || !g01 || !partials) return IAS_ERR_ARG;
  int nchunks = 0;
  const int st = gain_shape(B, T, &nchunks);
  if (st != IAS_OK) return st;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(gain_energy_kernel, dim3(nchunks, B), dim3(GAIN_THREADS), 0, stream, target, render, T, nchunks,
                     partials);
  hipLaunchKernelGGL(gain_solve_fold_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, partials, B, nchunks, g01);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
