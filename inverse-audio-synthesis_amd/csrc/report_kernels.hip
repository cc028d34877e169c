// Match report (MI355X / gfx950): the contract of ias_spectral_report in include/ias_hip_report.h
// (inverse-audio-synthesis_amd/report.py: spectral_report, Reporter; match_audio.py --report).  A streaming reduction: two
// [B, F, K] tensors are read once, nothing of a frame is kept.  Logs are __log2f (v_log_f32), as in
// mrstft_rows_partials_kernel; the row's floor keeps every argument a normal number.
//
// spectral_report_partials_kernel<CM>: grid (chunks of RP_GROUP_FRAMES frames, B), 4 waves; wave w of chunk g takes the
//   frames g 32 + w 8 .. + 7 one after the other, a rule in F alone.  Lane l takes bins l, l + 64, ... with plain dword
//   loads (consecutive lanes on consecutive floats: no alignment path, a row may start at any 4-byte phase).  A wave's
//   frames are one contiguous span, cut into blocks of at most RP_UNROLL x 64 bins that never cross a frame; the loads of
//   the next block (the next frame's first, at a frame's end) are issued before the current one is worked on.  A bin
//   past K is loaded as v = t = 0: both clamp to the floor, so it adds +0 to every sum and leaves the maximum alone.
//   Per lane: fp32 chains for sum d^2, sum |d|, sum (t - v)^2, sum t^2, the running maximum and, with a table, up to CM
//   dot products D[c, :] . d with D in LDS, padded to CM rows with zeros (consecutive lanes on consecutive floats: 32
//   banks, no conflict).  At a frame's end fixed exchanges (__shfl_xor: rp_wave_sums) fold the lanes, the roots are
//   taken, and the frame is added to the wave's fp64 sums; whether a frame counts is one ballot.  Each wave leaves its
//   6 sums in LDS; lane j of the workgroup adds sum j of the waves in order and writes it into the chunk's record.
//   CM = 0 (no table), 16 or 32 bounds the unrolled accumulators: n_coef <= CM.
// spectral_report_fold_kernel: 8 lanes per row, 8 rows per wave; lane j < 6 adds sum j of the row's records in chunk
//   order, 8 records loaded at a time, and lane j < 5 applies a, the divisors or the convergence quotient in fp64 and
//   writes out[b][j].
#include "ias_common.h"
#include <cmath>

#define RP_THREADS 256
#define RP_WAVES (RP_THREADS / 64)
#define RP_WAVE_FRAMES 8
#define RP_GROUP_FRAMES (RP_WAVES * RP_WAVE_FRAMES)     // 32 frames per workgroup and record
#define RP_UNROLL 4                                     // 64-bin steps per block
#define RP_BLOCK (RP_UNROLL * 64)
#define RP_REC 6                                        // {sum_f rms d, sum |d|, sum (t - v)^2, sum t^2, sum_f cepstral, n}
#define RP_MAX_BINS 2048
#define RP_MAX_COEF 32
#define RP_MAX_DCT_BINS 256

// The wave's sums of M values per lane (M a power of two, 2 .. 64) in M - 1 + 6 - log2 M exchanges instead of 6 M: at the
// step of lane bit m a lane hands the half of its values that the other side of the bit keeps to its partner and adds
// what it gets to the half it keeps; once one value is left the steps are plain butterflies.  On return x[0] of a lane
// is the sum over the wave of x[j], j = lane >> (6 - log2 M); the order of the additions is fixed.
template <int M, int S>
__device__ __forceinline__ void rp_wave_sums_step(float (&x)[M], int lane) {
  constexpr int m = 32 >> S;
  constexpr int half = M >> (S + 1);                     // values a lane keeps at this step; 0: one is left
  if constexpr (half >= 1) {
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = up ? x[i] : x[i + half];
      const float keep = up ? x[i + half] : x[i];
      x[i] = keep + __shfl_xor(send, m, 64);
    }
  } else {
    x[0] += __shfl_xor(x[0], m, 64);
  }
}

template <int M>
__device__ __forceinline__ float rp_wave_sums(float (&x)[M], int lane) {
  rp_wave_sums_step<M, 0>(x, lane);
  rp_wave_sums_step<M, 1>(x, lane);
  rp_wave_sums_step<M, 2>(x, lane);
  rp_wave_sums_step<M, 3>(x, lane);
  rp_wave_sums_step<M, 4>(x, lane);
  rp_wave_sums_step<M, 5>(x, lane);
  return x[0];
}

template <int CM>
__global__ __launch_bounds__(RP_THREADS) void spectral_report_partials_kernel(const float* __restrict__ values,
                                                                              const float* __restrict__ target,
                                                                              const float* __restrict__ floor_rows,
                                                                              const float* __restrict__ dct, int F, int K,
                                                                              int C, int nchunks,
                                                                              double* __restrict__ partials) {
  extern __shared__ double rp_lds[];                     // [RP_WAVES][RP_REC] doubles, then the table [CM][K] floats
  double* red = rp_lds;
  float* tab = (float*)(rp_lds + RP_WAVES * RP_REC);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = blockIdx.x, b = blockIdx.y;
  if (CM > 0) {
    for (int i = tid; i < CM * K; i += RP_THREADS) tab[i] = i < C * K ? dct[i] : 0.0f;   // rows C .. CM - 1: zeros
    __syncthreads();
  }
  const float fl = floor_rows[b];
  const int f0 = g * RP_GROUP_FRAMES + w * RP_WAVE_FRAMES;
  int nf = F - f0;                                       // the wave's frames: wave-uniform
  nf = nf < 0 ? 0 : (nf > RP_WAVE_FRAMES ? RP_WAVE_FRAMES : nf);
  const size_t span = ((size_t)b * F + (size_t)(nf > 0 ? f0 : 0)) * K;
  const float* vs = values + span;                       // frame i of the wave starts at i K
  const float* ts = target + span;

  // lane >> 4 says which of the four frame sums the lane adds up after rp_wave_sums<4>: 0 the rms of d, 1 sum |d|,
  // 2 sum (t - v)^2, 3 sum t^2
  const int mine = lane >> 4;
  double a_mine = 0.0, a_mcd = 0.0, a_n = 0.0;
  float s_d2 = 0.0f, s_l1 = 0.0f, s_num = 0.0f, s_den = 0.0f, s_max = 0.0f;
  float dc[CM > 0 ? CM : 2];
#pragma unroll
  for (int c = 0; c < (CM > 0 ? CM : 2); ++c) dc[c] = 0.0f;

  float vv[RP_UNROLL] = {}, tt[RP_UNROLL] = {}, vn[RP_UNROLL] = {}, tn[RP_UNROLL] = {};
  auto load = [&](int fi, int k0, float (&v)[RP_UNROLL], float (&t)[RP_UNROLL]) {
    const float* vf = vs + (size_t)fi * K;
    const float* tf = ts + (size_t)fi * K;
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
      const int k = k0 + u * 64 + lane;
      const bool ok = k < K;
      v[u] = ok ? vf[k] : 0.0f;
      t[u] = ok ? tf[k] : 0.0f;
    }
  };

  int fi = 0, k0 = 0;                                    // the block in vv / tt
  if (nf > 0) load(0, 0, vv, tt);
  while (fi < nf) {
    int fn = fi, kn = k0 + RP_BLOCK;                     // the block behind it
    if (kn >= K) {
      kn = 0;
      ++fn;
    }
    if (fn < nf) load(fn, kn, vn, tn);
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
      if (k0 + u * 64 < K) {                             // wave-uniform: no work on a step that is past K as a whole
        const float v = vv[u], t = tt[u];
        s_max = fmaxf(s_max, fmaxf(v, t));
        const float e = t - v;
        s_num = fmaf(e, e, s_num);
        s_den = fmaf(t, t, s_den);
        const float d = __log2f(fmaxf(v, fl)) - __log2f(fmaxf(t, fl));
        s_d2 = fmaf(d, d, s_d2);
        s_l1 += fabsf(d);
        if (CM > 0) {
          int k = k0 + u * 64 + lane;                    // a lane past K has d = 0: any finite entry of the table will do
          k = k < K ? k : K - 1;
#pragma unroll
          for (int c = 0; c < CM; ++c) dc[c] = fmaf(tab[c * K + k], d, dc[c]);
        }
      }
    }
    if (fn != fi) {                                      // the frame is complete
      float x4[4] = {s_d2, s_l1, s_num, s_den};
      const float sum = rp_wave_sums<4>(x4, lane);
      a_mine += (double)(mine == 0 ? sqrtf(sum / (float)K) : sum);
      a_n += __any(s_max > fl) ? 1.0 : 0.0;
      if (CM > 0) {
        const float s = rp_wave_sums<(CM > 0 ? CM : 2)>(dc, lane);      // coefficient lane >> (6 - log2 CM); 0 from C on
        float q = s * s;
#pragma unroll
        for (int m = 32; m >= 64 / (CM > 0 ? CM : 2); m >>= 1) q += __shfl_xor(q, m, 64);   // over the coefficients
        a_mcd += (double)sqrtf(2.0f * q);
#pragma unroll
        for (int c = 0; c < CM; ++c) dc[c] = 0.0f;
      }
      s_d2 = s_l1 = s_num = s_den = s_max = 0.0f;
    }
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
      vv[u] = vn[u];
      tt[u] = tn[u];
    }
    fi = fn;
    k0 = kn;
  }

  double* r = red + w * RP_REC;
  if ((lane & 15) == 0) r[mine] = a_mine;
  if (lane == 0) r[4] = a_mcd, r[5] = a_n;
  __syncthreads();
  if (tid < RP_REC) {                                    // lane j adds sum j of the waves in wave order
    double s = red[tid];
    for (int ww = 1; ww < RP_WAVES; ++ww) s += red[ww * RP_REC + tid];
    partials[((size_t)b * nchunks + g) * RP_REC + tid] = s;
  }
}

#define RP_FOLD_ROWS 8                                  // rows per wave of the fold: 8 lanes each, 6 of them at work
#define RP_FOLD_AHEAD 8                                 // records loaded before they are added

__global__ __launch_bounds__(64) void spectral_report_fold_kernel(const double* __restrict__ partials, int B, int nchunks,
                                                                 int K, int power, int has_dct,
                                                                 double* __restrict__ out) {
  const int lane = threadIdx.x, j = lane & 7;
  const int b = blockIdx.x * RP_FOLD_ROWS + (lane >> 3);
  const bool live = b < B && j < RP_REC;
  const double* p = partials + ((size_t)(live ? b : 0) * nchunks) * RP_REC + (live ? j : 0);
  double s = 0.0;                                        // sum j of the row, its records added in chunk order
  for (int c0 = 0; c0 < nchunks; c0 += RP_FOLD_AHEAD) {
    double x[RP_FOLD_AHEAD];
#pragma unroll
    for (int u = 0; u < RP_FOLD_AHEAD; ++u) x[u] = (live && c0 + u < nchunks) ? p[(size_t)(c0 + u) * RP_REC] : 0.0;
#pragma unroll
    for (int u = 0; u < RP_FOLD_AHEAD; ++u) s += x[u];   // + 0.0 past the end: the sums are >= +0, their bits stay
  }
  double r[RP_REC];
#pragma unroll
  for (int i = 0; i < RP_REC; ++i) r[i] = __shfl(s, (lane & ~7) + i, 64);
  const double a = (20.0 / (double)power) * 0.30102999566398119521;          // log10 2
  const double n = r[5];
  double o = n;
  if (j == 0) o = n > 0.0 ? a * r[0] / n : 0.0;
  if (j == 1) o = r[3] > 0.0 ? sqrt(r[2]) / sqrt(r[3]) : (r[2] > 0.0 ? (double)INFINITY : 0.0);
  if (j == 2) o = n > 0.0 ? a * r[1] / (n * (double)K) : 0.0;
  if (j == 3) o = (has_dct && n > 0.0) ? 0.5 * a * r[4] / n : 0.0;            // (10 / ln 10) (ln 2 / power) = a / 2
  if (b < B && j < 5) out[(size_t)b * 5 + j] = o;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ias_report_build_dct(int n_in, int n_coef, float* out_host) {
  if (!out_host || n_in < 1 || n_coef < 1) return IAS_ERR_ARG;
  if (n_coef >= n_in) return IAS_ERR_UNSUPPORTED;
  const double pi = 3.14159265358979323846;
  const double scale = sqrt(2.0 / (double)n_in);
  for (int c = 1; c <= n_coef; ++c)
    for (int k = 0; k < n_in; ++k)
      out_host[(size_t)(c - 1) * n_in + k] =
          (float)(scale * cos(pi * (double)c * (double)(2 * k + 1) / (double)(2 * n_in)));
  return IAS_OK;
}

extern "C" long long ias_spectral_report_partials_count(int F) {
  if (F < 1) return IAS_ERR_ARG;
  return ((long long)F + RP_GROUP_FRAMES - 1) / RP_GROUP_FRAMES;
}

extern "C" int ias_spectral_report(const float* values, const float* target, const float* floor_rows, const float* dct,
                                   int B, int F, int K, int n_coef, int power, double* partials, double* out,
                                   void* stream_) {
  if (!values || !target || !floor_rows || !partials || !out) return IAS_ERR_ARG;
  if (B < 1 || F < 1 || K < 1) return IAS_ERR_ARG;
  if (power != 1 && power != 2) return IAS_ERR_ARG;
  if (dct && n_coef < 1) return IAS_ERR_ARG;
  if (B > 65535 || K > RP_MAX_BINS) return IAS_ERR_UNSUPPORTED;
  if (dct && (n_coef > RP_MAX_COEF || n_coef >= K || K > RP_MAX_DCT_BINS)) return IAS_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  const int nchunks = (int)ias_spectral_report_partials_count(F);
  const int C = dct ? n_coef : 0;
  const dim3 grid((unsigned)nchunks, (unsigned)B);
  const int CM = C == 0 ? 0 : (C <= 16 ? 16 : 32);       // the table in LDS is padded with rows of zeros to CM
  const size_t lds = (size_t)RP_WAVES * RP_REC * 8 + (size_t)CM * K * 4;
  if (C == 0)
    hipLaunchKernelGGL(spectral_report_partials_kernel<0>, grid, dim3(RP_THREADS), lds, stream, values, target,
                       floor_rows, dct, F, K, C, nchunks, partials);
  else if (C <= 16)
    hipLaunchKernelGGL(spectral_report_partials_kernel<16>, grid, dim3(RP_THREADS), lds, stream, values, target,
                       floor_rows, dct, F, K, C, nchunks, partials);
  else
    hipLaunchKernelGGL(spectral_report_partials_kernel<32>, grid, dim3(RP_THREADS), lds, stream, values, target,
                       floor_rows, dct, F, K, C, nchunks, partials);
  if (hipGetLastError() != hipSuccess) return IAS_ERR_LAUNCH;
  hipLaunchKernelGGL(spectral_report_fold_kernel, dim3((unsigned)((B + RP_FOLD_ROWS - 1) / RP_FOLD_ROWS)), dim3(64), 0,
                     stream, partials, B, nchunks, K, power, C > 0 ? 1 : 0, out);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
