// Onset detection and note segmentation of sound matching (MI355X / gfx950): the contracts of ias_onset_flux,
// ias_onset_pick, ias_segment_gather and ias_segment_scatter in include/ias_hip.h (inverse-audio-synthesis_amd/onset.py,
// match_audio.py --split).  Built with -ffp-contract=off (Makefile): every fp64 step and the fades' two fp32 products
// round where the contract says.
//
// onset_flux_kernel: one workgroup of 256 lanes per OF_FRAMES = 16 consecutive frames of a row, 1-D grid.  The mels are
//   walked in chunks of OF_CHUNK = 256.  Per chunk every lane takes elements (frame, m) of the tile with m fastest, so a
//   wave reads consecutive floats of mel; it forms L of the element and of the same mel `lag` frames earlier (log1p in
//   fp64, each rounded to fp32 once; +0 before the row's first frame), the exact fp64 difference and its positive part,
//   which goes to LDS as d[m][frame] (row pitch 17 doubles).  Then lane f < 16 continues frame f's chain over the chunk in
//   ascending m: the 16 lanes read 16 consecutive doubles per step.  L of a frame is computed twice, once as the current
//   and once as the lagged frame, by the same instruction sequence on the same input: the same bits.  That keeps the
//   kernel free of a limit on lag and M; the mel tensor is read twice (the second time from L2: the lagged tile is the
//   tile of a neighbouring workgroup), against fp64 log1p work of the same order as the tensor's HBM time.
// onset_pick_kernel: one workgroup of 1024 lanes per row.  Frames are walked in chunks of 1024: a lane evaluates its
//   frame's two window conditions from global memory (a row of flux is 4 F bytes and stays in L2), every wave leaves the
//   ballot of its 64 flags in LDS (two buffers: one barrier per chunk), and lane 0 walks the set bits of the previous
//   chunk's 16 words in ascending order (the compacted candidates) with the greedy `wait` rule while the other lanes are
//   already at the next chunk's windows.
// segment_copy_kernel<SCATTER>: both directions of the copy between audio [N, L] at (row[s], start[s] + t) and the note
//   buffers [S, T] at (s, t).  A lane owns one 16-byte-aligned group of four floats of the STORE side; when the load
//   side of the group has the same 16-byte phase it is one dwordx4 load, otherwise four dword loads.  Groups that cross
//   an end of the valid range fall back to element-wise access with every index checked, so nothing outside [0, L) of
//   a row in [0, N) and nothing outside [0, T) of a note is ever touched.
#include "ias_common.h"
#include <climits>
#include <cmath>
#include <cstdint>

#define OF_THREADS 256
#define OF_FRAMES 16
#define OF_CHUNK 256
#define OF_PITCH (OF_FRAMES + 1)
#define OP_THREADS 1024
#define OP_WAVES (OP_THREADS / 64)
#define SG_THREADS 256

__device__ __forceinline__ float onset_logmel(float mel, double gamma) { return (float)log1p(gamma * (double)mel); }

__global__ __launch_bounds__(OF_THREADS) void onset_flux_kernel(const float* __restrict__ mel, int F, int M, int lag,
                                                                float gamma_, int tiles, float* __restrict__ flux,
                                                                float* __restrict__ logmel) {
  __shared__ double d[OF_CHUNK * OF_PITCH];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / tiles, f0 = (blockIdx.x % tiles) * OF_FRAMES;
  const int nf = F - f0 < OF_FRAMES ? F - f0 : OF_FRAMES;
  const double gamma = (double)gamma_;
  const size_t row = (size_t)b * F;
  double acc = 0.0;
  for (int m0 = 0; m0 < M; m0 += OF_CHUNK) {
    const int mc = M - m0 < OF_CHUNK ? M - m0 : OF_CHUNK;
    for (int i = tid; i < nf * mc; i += OF_THREADS) {
      const int fl = i / mc, ml = i - fl * mc;
      const int f = f0 + fl;
      const size_t at = (row + f) * (size_t)M + (size_t)(m0 + ml);
      const float cur = onset_logmel(mel[at], gamma);
      const float prev = f >= lag ? onset_logmel(mel[at - (size_t)lag * M], gamma) : 0.0f;
      if (logmel) logmel[at] = cur;
      const double diff = (double)cur - (double)prev;
      d[ml * OF_PITCH + fl] = diff > 0.0 ? diff : 0.0;
    }
    __syncthreads();
    if (tid < nf)
      for (int ml = 0; ml < mc; ++ml) acc += d[ml * OF_PITCH + tid];
    __syncthreads();
  }
  if (tid < nf) flux[row + f0 + tid] = (float)(acc / (double)M);
}

__global__ __launch_bounds__(OP_THREADS) void onset_pick_kernel(const float* __restrict__ flux, int F, int pre_max,
                                                                int post_max, int pre_avg, int post_avg, float delta_,
                                                                int wait, int K, int* __restrict__ frames,
                                                                float* __restrict__ strength, int* __restrict__ count) {
  __shared__ unsigned long long s_mask[2][OP_WAVES];
  __shared__ int s_count;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int b = blockIdx.x;
  const float* x = flux + (size_t)b * F;
  int* fr = frames + (size_t)b * K;
  float* sg = strength + (size_t)b * K;
  const double delta = (double)delta_;
  const int chunks = (F + OP_THREADS - 1) / OP_THREADS;
  int accepted = 0, last = 0;                            // lane 0's walk
  for (int c = 0; c <= chunks; ++c) {
    if (c < chunks) {
      const int f = c * OP_THREADS + tid;
      bool cand = false;
      if (f < F) {
        const float v = x[f];
        cand = true;
        const int lo = pre_max > f ? 0 : f - pre_max, hi = post_max < F - 1 - f ? f + post_max : F - 1;
        for (int g = lo; g <= hi; ++g) cand = cand && (v >= x[g]);
        const int alo = pre_avg > f ? 0 : f - pre_avg, ahi = post_avg < F - 1 - f ? f + post_avg : F - 1;
        double s = 0.0;
        for (int g = alo; g <= ahi; ++g) s += (double)x[g];
        const double mean = s / (double)(ahi - alo + 1);
        cand = cand && ((double)v >= mean + delta);
      }
      const unsigned long long m = __ballot(cand);
      if ((tid & 63) == 0) s_mask[c & 1][wave] = m;
    }
    __syncthreads();
    if (tid == 0 && c < chunks) {
      for (int w = 0; w < OP_WAVES; ++w) {
        unsigned long long m = s_mask[c & 1][w];
        while (m) {
          const int f = c * OP_THREADS + w * 64 + __builtin_ctzll(m);
          m &= m - 1;
          if (accepted == 0 || f - last > wait) {
            if (accepted < K) {
              fr[accepted] = f;
              sg[accepted] = x[f];
            }
            if (accepted < INT_MAX) ++accepted;
            last = f;
          }
        }
      }
      if (c == chunks - 1) s_count = accepted;
    }
  }
  // the loop's last pass (c == chunks) is a barrier alone: s_count is visible to every lane
  const int n = s_count;
  for (int k = (n < K ? n : K) + tid; k < K; k += OP_THREADS) {
    fr[k] = -1;
    sg[k] = 0.0f;
  }
  if (tid == 0) count[b] = n;
}

// The fade factor of sample t of a note of `length` samples: 1 outside the last `fade` samples of a faded note.
__device__ __forceinline__ float segment_fade(float v, int t, int length, int fade, float inv_fade, bool faded) {
  if (faded && t >= length - fade) return v * ((float)(length - t) * inv_fade);
  return v;
}

template <bool SCATTER>
__global__ __launch_bounds__(SG_THREADS) void segment_copy_kernel(const float* __restrict__ src, int N, int L,
                                                                  const int* __restrict__ row_, const int* __restrict__ start_,
                                                                  const int* __restrict__ length_,
                                                                  const unsigned char* __restrict__ faded_, int T, int fade,
                                                                  float inv_fade, const float* __restrict__ gain_,
                                                                  float* __restrict__ dst, int tiles) {
  const int s = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int r = row_[s], length = length_[s];
  const long long start = start_[s];
  const bool faded = faded_[s] != 0;
  const bool row_ok = r >= 0 && r < N;
  const int n = length < 0 ? 0 : (length < T ? length : T);          // samples of the note that carry audio
  const float gain = SCATTER ? gain_[s] : 1.0f;
  if (SCATTER && !row_ok) return;
  // a: the audio side (row r, sample start + t), may be out of range; n: the note side (note s, sample t)
  const float* a_rd = SCATTER ? nullptr : src + (size_t)(row_ok ? r : 0) * L;
  float* a_wr = SCATTER ? dst + (size_t)r * L : nullptr;
  const float* n_rd = SCATTER ? src + (size_t)s * T : nullptr;
  float* n_wr = SCATTER ? nullptr : dst + (size_t)s * T;
  // word address (in floats) of the store side's and the load side's sample t = 0; only their low two bits matter
  const long long st_w = SCATTER ? (long long)((uintptr_t)a_wr >> 2) + start : (long long)((uintptr_t)n_wr >> 2);
  const long long ld_w = SCATTER ? (long long)((uintptr_t)n_rd >> 2) : (long long)((uintptr_t)a_rd >> 2) + start;
  const int t0 = 4 * (tile * SG_THREADS + (int)threadIdx.x) - (int)(st_w & 3);   // the group's first sample: 16-byte aligned store
  const int t_end = SCATTER ? n : T;                                 // samples t the store side covers: [0, t_end)
  if (t0 >= t_end || t0 + 3 < 0) return;
  const bool whole = t0 >= 0 && t0 + 3 < t_end;
  float v[4];
  // the load: in one piece when the four samples exist and the load side is aligned too
  const bool ld_all = SCATTER ? whole : (row_ok && t0 >= 0 && t0 + 3 < n && start + t0 >= 0 && start + t0 + 3 < (long long)L);
  if (ld_all && ((ld_w + t0) & 3) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(SCATTER ? n_rd + t0 : a_rd + (start + t0));
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + j;
      const long long i = start + t;
      bool ok = t >= 0 && t < n;
      if (!SCATTER) ok = ok && row_ok && i >= 0 && i < (long long)L;
      v[j] = ok ? (SCATTER ? n_rd[t] : a_rd[i]) : 0.0f;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = t0 + j;
    if (SCATTER) v[j] = v[j] * gain;
    if (t >= 0 && t < n) v[j] = segment_fade(v[j], t, length, fade, inv_fade, faded);
  }
  if (SCATTER) {
    if (whole && start + t0 >= 0 && start + t0 + 3 < (long long)L) {
      *reinterpret_cast<float4*>(a_wr + (start + t0)) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = t0 + j;
        const long long i = start + t;
        if (t >= 0 && t < n && i >= 0 && i < (long long)L) a_wr[i] = v[j];
      }
    }
  } else {
    if (whole) {
      *reinterpret_cast<float4*>(n_wr + t0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = t0 + j;
        if (t >= 0 && t < T) n_wr[t] = v[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ias_onset_flux(const float* mel, int B, int F, int M, int lag, float gamma, float* flux, float* logmel,
                              void* stream_) {
  if (!mel || !flux) return IAS_ERR_ARG;
  if (B < 1 || F < 1 || M < 1 || lag < 1) return IAS_ERR_ARG;
  if (!(gamma > 0.0f) || !std::isfinite(gamma)) return IAS_ERR_ARG;             // a NaN is refused too
  const int tiles = (F + OF_FRAMES - 1) / OF_FRAMES;
  if ((long long)B * tiles > (long long)INT_MAX) return IAS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(onset_flux_kernel, dim3((unsigned)(B * tiles)), dim3(OF_THREADS), 0, (hipStream_t)stream_, mel, F, M,
                     lag, gamma, tiles, flux, logmel);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_onset_pick(const float* flux, int B, int F, int pre_max, int post_max, int pre_avg, int post_avg,
                              float delta, int wait, int K, int* frames, float* strength, int* count, void* stream_) {
  if (!flux || !frames || !strength || !count) return IAS_ERR_ARG;
  if (B < 1 || F < 1 || K < 1) return IAS_ERR_ARG;
  if (pre_max < 0 || post_max < 0 || pre_avg < 0 || post_avg < 0 || wait < 0) return IAS_ERR_ARG;
  if (!(delta > 0.0f)) return IAS_ERR_ARG;                                      // a NaN is refused too
  if (B > 65535) return IAS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(onset_pick_kernel, dim3((unsigned)B), dim3(OP_THREADS), 0, (hipStream_t)stream_, flux, F, pre_max,
                     post_max, pre_avg, post_avg, delta, wait, K, frames, strength, count);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

// Workgroups of a segment copy: a note's T samples are at most (T + 3) / 4 + 1 aligned groups of the store side.
static long long segment_tiles(int T) { return ((long long)T / 4 + 2 + SG_THREADS - 1) / SG_THREADS; }

extern "C" int ias_segment_gather(const float* audio, int N, int L, const int* row, const int* start, const int* length,
                                  const unsigned char* faded, int S, int T, int fade, float inv_fade, float* out,
                                  void* stream_) {
  if (!audio || !row || !start || !length || !faded || !out) return IAS_ERR_ARG;
  if (N < 1 || L < 1 || S < 1 || T < 1 || fade < 0 || !std::isfinite(inv_fade)) return IAS_ERR_ARG;
  const long long tiles = segment_tiles(T);
  if (T > INT_MAX - 8 * SG_THREADS || (long long)S * tiles > (long long)INT_MAX) return IAS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(segment_copy_kernel<false>, dim3((unsigned)(S * tiles)), dim3(SG_THREADS), 0, (hipStream_t)stream_,
                     audio, N, L, row, start, length, faded, T, fade, inv_fade, (const float*)nullptr, out, (int)tiles);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}

extern "C" int ias_segment_scatter(const float* notes, int N, int L, const int* row, const int* start, const int* length,
                                   const unsigned char* faded, int S, int T, int fade, float inv_fade, const float* gain,
                                   float* out, void* stream_) {
  if (!notes || !row || !start || !length || !faded || !gain || !out) return IAS_ERR_ARG;
  if (N < 1 || L < 1 || S < 1 || T < 1 || fade < 0 || !std::isfinite(inv_fade)) return IAS_ERR_ARG;
  const long long tiles = segment_tiles(T);
  if (T > INT_MAX - 8 * SG_THREADS || (long long)S * tiles > (long long)INT_MAX) return IAS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(segment_copy_kernel<true>, dim3((unsigned)(S * tiles)), dim3(SG_THREADS), 0, (hipStream_t)stream_,
                     notes, N, L, row, start, length, faded, T, fade, inv_fade, gain, out, (int)tiles);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
