// Pitch estimator of sound matching (MI355X / gfx950): YIN (de Cheveigne & Kawahara 2002) per frame of every target row,
// the contract of ias_pitch_yin in include/ias_hip.h (inverse-audio-synthesis_amd/pitch.py: pitch_yin, estimate_pitch).
// Built with -ffp-contract=off (Makefile): the difference function is an explicit fmaf chain and the fp64 steps behind it
// are rounded where the contract says.
//
// pitch_yin_kernel: one workgroup per (frame f, row b), grid (F, B), 64..256 lanes.  LDS (dynamic): c [tau_max + 1] fp64,
//   the frame x [W + tau_max] fp32 followed by PY_PAD zeros, d [tau_max + 1] fp32.
//   1. The workgroup stages the frame's W + tau_max samples once (plain dword loads: a row starts at any 4-byte phase).
//   2. Difference function.  A lane owns PY_R = 7 consecutive lags t0 .. t0 + 6, t0 = 1 + 7 blk, blk = lane, lane + lanes,
//      ...; it keeps the seven accumulators and a seven-register window of x[j + t0 ..] that slides by one sample per j,
//      so a j costs one broadcast read of x[j], ONE new ds_read_b32 and 7 (v_sub_f32 + v_fma_f32).  The j loop is unrolled
//      by 7, which makes the window's rotation a renaming of registers.  Lane l reads dword j + t0 + 7 + u, stride 7
//      between lanes: 7 is odd, so the 32 lanes of a ds_read_b32 group land in 32 different banks.  Every lag still sees
//      j = 0 .. W - 1 in order, one chain from +0.  Lags past tau_max in a lane's last block read the zero padding and
//      are not stored.  The last lane then takes the frame's energy, the same chain over x[j]^2.
//   3. Lane 0 forms the running sum c(tau) in fp64 in tau order into LDS (a serial chain by contract).
//   4. All lanes turn d into d' in place (one fp64 multiply and divide per lag, rounded once to fp32), copy it out when
//      the caller asked for it, and leave the first lag under the threshold and the first global minimum in two LDS words
//      (atomic min on tau, and on the pair (bits of d', tau): d' >= 0, so its bit pattern orders as its value).
//   5. Lane 0 walks to the local minimum, refines it by a parabola in fp64 and writes period and aperiodicity.
//   One launch, no workspace, no global atomics; a frame's outputs are a function of its samples and the scalars alone.
#include "ias_common.h"
#include <climits>

#define PY_R 7                     // lags per lane: odd (bank rule above)
#define PY_PAD 8                   // zeros behind the frame: a lane's last block reads up to PY_R dwords past it
#define PY_THREADS 256
#define PY_LDS_BYTES 65536         // the kernel's LDS budget (include/ias_hip.h)

static inline long long py_lds_bytes(int W, int tau_max) {
  return 8LL * (tau_max + 1LL) + 4LL * ((long long)W + tau_max + PY_PAD) + 4LL * (tau_max + 1LL);
}

__global__ __launch_bounds__(PY_THREADS) void pitch_yin_kernel(const float* __restrict__ audio, int T, int W, int tau_min,
                                                               int tau_max, int hop, float threshold,
                                                               float* __restrict__ period, float* __restrict__ aperiodicity,
                                                               float* __restrict__ energy, float* __restrict__ dprime) {
  extern __shared__ double py_lds[];
  __shared__ int s_first;                                // smallest tau in [tau_min, tau_max] with d' < threshold
  __shared__ unsigned long long s_min;                   // min over [tau_min, tau_max] of (bits of d') << 32 | tau
  const int L = W + tau_max;
  double* cl = py_lds;
  float* xs = (float*)(cl + tau_max + 1);
  float* dl = xs + L + PY_PAD;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int f = blockIdx.x, b = blockIdx.y, F = gridDim.x;
  const float* x = audio + (size_t)b * T + (size_t)f * hop;

  for (int i = tid; i < L + PY_PAD; i += nt) xs[i] = i < L ? x[i] : 0.0f;
  if (tid == 0) {
    dl[0] = 0.0f;
    s_first = INT_MAX;
    s_min = ~0ull;
  }
  __syncthreads();

  for (int blk = tid; blk * PY_R < tau_max; blk += nt) {
    const int t0 = 1 + blk * PY_R;
    const float* xw = xs + t0;
    float w[PY_R], acc[PY_R];
#pragma unroll
    for (int i = 0; i < PY_R; ++i) {
      w[i] = xw[i];
      acc[i] = 0.0f;
    }
    // slot k of w holds x[j + t0 + k] for k >= u and x[j + t0 + 7 + k] for k < u: lag t0 + i reads slot (u + i) mod 7
    int j = 0;
    for (; j + PY_R <= W; j += PY_R) {
#pragma unroll
      for (int u = 0; u < PY_R; ++u) {
        const float xj = xs[j + u];
#pragma unroll
        for (int i = 0; i < PY_R; ++i) {
          const float d = xj - w[(u + i) % PY_R];
          acc[i] = fmaf(d, d, acc[i]);
        }
        w[u] = xw[j + u + PY_R];
      }
    }
#pragma unroll
    for (int u = 0; u < PY_R - 1; ++u) {
      if (j + u >= W) break;
      const float xj = xs[j + u];
#pragma unroll
      for (int i = 0; i < PY_R; ++i) {
        const float d = xj - w[(u + i) % PY_R];
        acc[i] = fmaf(d, d, acc[i]);
      }
      w[u] = xw[j + u + PY_R];
    }
#pragma unroll
    for (int i = 0; i < PY_R; ++i)
      if (t0 + i <= tau_max) dl[t0 + i] = acc[i];
  }
  if (tid == nt - 1) {
    float e = 0.0f;
    for (int j = 0; j < W; ++j) e = fmaf(xs[j], xs[j], e);
    energy[(size_t)b * F + f] = e;
  }
  __syncthreads();

  if (tid == 0) {
    double c = 0.0;
    cl[0] = 0.0;
    for (int t = 1; t <= tau_max; ++t) {
      c += (double)dl[t];
      cl[t] = c;
    }
  }
  __syncthreads();

  float* dp_out = dprime ? dprime + ((size_t)b * F + f) * (size_t)(tau_max + 1) : nullptr;
  int first = INT_MAX;
  unsigned long long best = ~0ull;
  for (int t = tid; t <= tau_max; t += nt) {
    const double c = cl[t];
    const float v = (t == 0 || c == 0.0) ? 1.0f : (float)((double)dl[t] * (double)t / c);
    dl[t] = v;
    if (dp_out) dp_out[t] = v;
    if (t >= tau_min) {
      if (v < threshold && t < first) first = t;
      const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)t;
      best = key < best ? key : best;
    }
  }
  if (first != INT_MAX) atomicMin(&s_first, first);
  if (best != ~0ull) atomicMin(&s_min, best);
  __syncthreads();

  if (tid == 0) {
    int t = s_first;
    if (t == INT_MAX) {
      t = (int)(s_min & 0xffffffffull);                  // some tau in [tau_min, tau_max]: the range is never empty
    } else {
      while (t + 1 <= tau_max && dl[t + 1] < dl[t]) ++t;
    }
    const float y1f = dl[t];
    float p = (float)t;
    if (t > tau_min && t < tau_max) {
      const double y0 = (double)dl[t - 1], y1 = (double)y1f, y2 = (double)dl[t + 1];
      const double den = y0 - 2.0 * y1 + y2;
      if (den > 0.0) p = (float)((double)t + (y0 - y2) / (2.0 * den));
    }
    period[(size_t)b * F + f] = p;
    aperiodicity[(size_t)b * F + f] = y1f;
  }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" long long ias_pitch_frames(int T, int W, int tau_max, int hop) {
  if (T < 1 || W < 1 || tau_max < 1 || hop < 1) return IAS_ERR_ARG;
  const long long span = (long long)W + tau_max;
  if ((long long)T < span) return IAS_ERR_ARG;
  return ((long long)T - span) / hop + 1;
}

extern "C" int ias_pitch_yin(const float* audio, int B, int T, int W, int tau_min, int tau_max, int hop, float threshold,
                             float* period, float* aperiodicity, float* energy, float* dprime, void* stream_) {
  if (!audio || !period || !aperiodicity || !energy) return IAS_ERR_ARG;
  if (B < 1 || T < 1 || W < 1 || hop < 1 || tau_min < 2 || tau_min > tau_max) return IAS_ERR_ARG;
  if (!(threshold > 0.0f && threshold <= 1.0f)) return IAS_ERR_ARG;           // a NaN is refused too
  const long long F = ias_pitch_frames(T, W, tau_max, hop);
  if (F < 1) return IAS_ERR_ARG;
  const long long lds = py_lds_bytes(W, tau_max);
  if (lds > PY_LDS_BYTES || B > 65535) return IAS_ERR_UNSUPPORTED;
  if (dprime && (long long)B * F > (long long)INT_MAX / (tau_max + 1)) return IAS_ERR_UNSUPPORTED;
  const int blocks = (tau_max + PY_R - 1) / PY_R;                            // lag blocks of a frame, one per lane and pass
  int threads = ((blocks + 63) / 64) * 64;
  threads = threads > PY_THREADS ? PY_THREADS : threads;
  hipLaunchKernelGGL(pitch_yin_kernel, dim3((unsigned)F, (unsigned)B), dim3(threads), (size_t)lds, (hipStream_t)stream_,
                     audio, T, W, tau_min, tau_max, hop, threshold, period, aperiodicity, energy, dprime);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
