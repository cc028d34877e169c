// Evolutionary search stage of sound matching (MI355X / gfx950): the two device primitives an elitist cross-entropy search
// (inverse-audio-synthesis_amd/evolve.py: evolve_search) needs beside ias_l1_cdist (scoring) and ias_topk_merge
// (selection, csrc/bank_kernels.hip): drawing a population around a per-sound mean and refitting the mean and the spread to
// the elites.  Both are one launch per generation and touch N M P and N k P floats: what they cost is a launch.
// Built with -ffp-contract=off (Makefile): the contracts in include/ias_hip.h fix every rounding point.
//
// evolve_sample_kernel (ias_evolve_sample): one lane per (sound n, candidate m, group q of four columns); grid (ceil(M G /
//   256), min(N, 65535)) with G = ceil(P / 4), the sounds of a launch with N > 65535 walked in a grid-stride loop.  The
//   lane runs Philox4x32-10 once on the counter (m_base + m, n_base + n, generation, q) under the key (seed lo, seed hi),
//   turns the four words into four standard normals by Box-Muller and writes columns 4 q .. 4 q + 3 (those below P).  The
//   counter names the value, not the lane: nothing depends on N, M, the grid or the cut of a population into calls.
// evolve_update_kernel (ias_evolve_update): one workgroup of 128 lanes per sound, lane j owns column j.  Lanes e < k first
//   resolve where elite e's parameters live (the generation's block, a slot of the previous elites, nowhere) into LDS; then
//   every lane copies its column of the k elites and, for a free column, takes the fp64 mean and variance over the valid
//   elites in slot order (two passes; the second reads the lane's own stores back) and blends them into mean and sigma.
//   No atomics: a sound belongs to one workgroup, a column to one lane.
#include "ias_common.h"
#include <cstdint>

#define EV_THREADS 256
#define EV_PMAX 128
#define EV_KMAX 64

// ------------------------------------------------------------------------------------------------ Philox4x32-10
struct EvWords { unsigned x0, x1, x2, x3; };

__device__ __forceinline__ EvWords ev_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}

// u(x) = ((x >> 9) + 0.5) 2^-23 = (2 (x >> 9) + 1) 2^-24: an odd 24-bit integer scaled by a power of two, exact, in (0, 1)
__device__ __forceinline__ float ev_unit(unsigned x) { return (float)(2u * (x >> 9) + 1u) * 5.9604644775390625e-08f; }

__device__ __forceinline__ void ev_box_muller(unsigned xa, unsigned xb, float& za, float& zb) {
  const float r = sqrtf(-2.0f * logf(ev_unit(xa)));
  const float t = 2.0f * ev_unit(xb);                    // exact; the pi-scaled functions take the turn count as it is
  za = r * cospif(t);
  zb = r * sinpif(t);
}

__global__ __launch_bounds__(EV_THREADS) void evolve_sample_kernel(const float* __restrict__ mean,
                                                                   const float* __restrict__ sigma,
                                                                   const unsigned char* __restrict__ free_cols, int N, int M,
                                                                   int P, unsigned n_base, unsigned long long m_base,
                                                                   unsigned key0, unsigned key1, unsigned generation,
                                                                   float* __restrict__ out) {
  const int G = (P + 3) >> 2;
  const long long t = (long long)blockIdx.x * EV_THREADS + threadIdx.x;
  if (t >= (long long)M * G) return;
  const int m = (int)(t / G), q = (int)(t % G);
  const unsigned cm = (unsigned)(m_base + (unsigned long long)m);        // < 2^32 (checked on the host)
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const EvWords w = ev_philox(cm, n_base + (unsigned)n, generation, (unsigned)q, key0, key1);
    float z[4];
    ev_box_muller(w.x0, w.x1, z[0], z[1]);
    ev_box_muller(w.x2, w.x3, z[2], z[3]);
    const float* mu = mean + (size_t)n * P;
    const float* sg = sigma + (size_t)n * P;
    float* o = out + ((size_t)n * M + m) * P;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * q + i;
      if (j >= P) break;
      float v = mu[j];
      if (free_cols[j]) {
        v = v + sg[j] * z[i];                            // one multiply, one add (no contraction in this file)
        v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);     // a NaN stays a NaN
      }
      o[j] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ distribution update
enum { EV_SRC_POP = 0, EV_SRC_PREV = 1, EV_SRC_ZERO = 2, EV_SRC_NAN = 3 };    // where an elite's parameters come from

__global__ __launch_bounds__(EV_PMAX) void evolve_update_kernel(const float* __restrict__ pop, long long base, int M,
                                                                const float* __restrict__ elite_dist,
                                                                const long long* __restrict__ elite_idx,
                                                                const long long* __restrict__ prev_idx,
                                                                const float* __restrict__ prev_params,
                                                                float* elite_params, float* mean, float* sigma,
                                                                const unsigned char* __restrict__ free_cols, int k, int P,
                                                                double alpha, double sigma_min, double sigma_max) {
  __shared__ int s_kind[EV_KMAX];
  __shared__ long long s_row[EV_KMAX];                   // the row of pop, or the slot of prev_params
  __shared__ unsigned char s_valid[EV_KMAX];
  const int n = blockIdx.x, tid = threadIdx.x;
  const long long* ei = elite_idx + (size_t)n * k;
  const long long* pi = prev_idx + (size_t)n * k;
  if (tid < k) {
    const long long ix = ei[tid];
    const unsigned du = __float_as_uint(elite_dist[(size_t)n * k + tid]);
    int kind = EV_SRC_NAN;
    long long row = 0;
    if (ix == INT64_MAX) {
      kind = EV_SRC_ZERO;
    } else if (ix >= base && ix - base < (long long)M) {
      kind = EV_SRC_POP;
      row = ix - base;
    } else {
      for (int s = 0; s < k; ++s)
        if (pi[s] == ix) { kind = EV_SRC_PREV; row = s; break; }
    }
    s_kind[tid] = kind;
    s_row[tid] = row;
    s_valid[tid] = ix != INT64_MAX && (du & 0x7f800000u) != 0x7f800000u;
  }
  __syncthreads();
  if (tid >= P) return;

  const float* popn = pop + (size_t)n * M * P;
  const float* prevn = prev_params + (size_t)n * k * P;
  float* en = elite_params + (size_t)n * k * P;
  const bool is_free = free_cols[tid] != 0;
  double sum = 0.0;
  int c = 0;
  for (int e = 0; e < k; ++e) {
    const int kind = s_kind[e];
    float x;
    if (kind == EV_SRC_POP) x = popn[(size_t)s_row[e] * P + tid];
    else if (kind == EV_SRC_PREV) x = prevn[(size_t)s_row[e] * P + tid];
    else if (kind == EV_SRC_ZERO) x = 0.0f;
    else x = __uint_as_float(0x7fc00000u);
    en[(size_t)e * P + tid] = x;
    if (s_valid[e]) { sum += (double)x; ++c; }
  }
  if (c == 0 || !is_free) return;
  const double mu = sum / (double)c;
  double var = 0.0;
  for (int e = 0; e < k; ++e) {
    if (!s_valid[e]) continue;
    const double d = (double)en[(size_t)e * P + tid] - mu;     // this lane's own store, read back
    var += d * d;
  }
  var = var / (double)c;
  const size_t at = (size_t)n * P + tid;
  double m2 = (1.0 - alpha) * (double)mean[at] + alpha * mu;
  m2 = m2 < 0.0 ? 0.0 : (m2 > 1.0 ? 1.0 : m2);
  double s2 = (1.0 - alpha) * (double)sigma[at] + alpha * sqrt(var);
  s2 = s2 < sigma_min ? sigma_min : s2;
  s2 = s2 > sigma_max ? sigma_max : s2;
  mean[at] = (float)m2;
  sigma[at] = (float)s2;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ias_evolve_sample(const float* mean, const float* sigma, const unsigned char* free_cols, int N, int M, int P,
                                 int n_base, long long m_base, unsigned long long seed, long long generation, float* out,
                                 void* stream_) {
  if (!mean || !sigma || !free_cols || !out) return IAS_ERR_ARG;
  if (N < 1 || M < 1 || P < 1 || P > EV_PMAX || n_base < 0 || m_base < 0 || generation < 0) return IAS_ERR_ARG;
  const long long lim = 1LL << 32;                       // every counter word is 32 bits
  if ((long long)n_base + N > lim || m_base > lim - M || generation >= lim) return IAS_ERR_UNSUPPORTED;
  const int G = (P + 3) >> 2;
  const long long blocks = ((long long)M * G + EV_THREADS - 1) / EV_THREADS;      // <= 2^28
  hipLaunchKernelGGL(evolve_sample_kernel, dim3((unsigned)blocks, (unsigned)(N < 65535 ? N : 65535)), dim3(EV_THREADS), 0,
                     (hipStream_t)stream_, mean, sigma, free_cols, N, M, P, (unsigned)n_base, (unsigned long long)m_base,
                     (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned)generation, out);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_evolve_update(const float* pop, long long base, int M, const float* elite_dist,
                                 const long long* elite_idx, const long long* prev_idx, const float* prev_params,
                                 float* elite_params, float* mean, float* sigma, const unsigned char* free_cols, int N,
                                 int k, int P, double alpha, double sigma_min, double sigma_max, void* stream_) {
  if (!pop || !elite_dist || !elite_idx || !prev_idx || !prev_params || !elite_params || !mean || !sigma || !free_cols)
    return IAS_ERR_ARG;
  if (N < 1 || M < 1 || k < 1 || k > EV_KMAX || P < 1 || P > EV_PMAX || base < 0) return IAS_ERR_ARG;
  if (!(alpha >= 0.0 && alpha <= 1.0) || !isfinite(sigma_min) || !isfinite(sigma_max) || sigma_min < 0.0 ||
      sigma_max < sigma_min)
    return IAS_ERR_ARG;
  if (elite_params == prev_params) return IAS_ERR_ARG;
  if (N > 65535) return IAS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(evolve_update_kernel, dim3(N), dim3(EV_PMAX), 0, (hipStream_t)stream_, pop, base, M, elite_dist,
                     elite_idx, prev_idx, prev_params, elite_params, mean, sigma, free_cols, k, P, alpha, sigma_min,
                     sigma_max);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
