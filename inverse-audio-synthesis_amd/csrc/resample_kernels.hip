// Band-limited resampling (MI355X / gfx950): torchaudio's windowed-sinc polyphase resampler
// (torchaudio.functional.resample: _get_sinc_resample_kernel + _apply_sinc_resample_kernel), the operation a reference user
// applies to audio at another rate before sound matching (inverse-audio-synthesis_amd/resample.py, match_audio.py
// --resample).
//
// With o = orig / g, n = new / g (g = gcd), the output is cut into blocks of n samples; block b, phase j is
//   y[b n + j] = sum_{i < K} xpad[b o + i] tap[j][i],   xpad[p] = x[p - width] inside the row, 0 outside,
// a strided correlation with n filters of K = 2 width + o taps (the table ias_resample_build_taps fills).
//
// Summation order (the per-row contract): every output is one fp32 fmaf chain over i = 0, 1, ..., K - 1 starting from
// +0.0f.  Nothing in it depends on B, the row's position, the span a workgroup owns or where the row sits in memory (x is
// read element by element), so an output is the same bits in every launch.
//
// resample_kernel<J>: grid (spans, rows), 256 lanes.  A workgroup owns `span` (<= 64) consecutive output blocks of one row
//   and stages their input window, (span - 1 + nq) o floats with nq = ceil(K / o), in LDS once; each input sample is read
//   from HBM about once.  The window is stored in rows of o samples with a row stride ostr = o | 1: lane l reads sample
//   l o + i at (l + i / o) ostr + i % o, and an odd stride puts the 64 lanes of a wave in 64 different banks.  A wave takes
//   groups of J phases in turn; lane l computes block l of the span for those J phases, so the taps it multiplies are the
//   same for all lanes (scalar loads from the table, which stays in L2) and each LDS read feeds J FMAs.
#include "ias_common.h"
#include <climits>

#define RS_THREADS 256
#define RS_SPAN 64                      // output blocks per workgroup: one per lane of a wave
#define RS_LDS_FLOATS 16384             // 64 KB of staged input per workgroup at most
#define RS_TAP_CAP (16LL << 20)         // taps in a table (n K), 64 MB
#define RS_MAX_ROWS 65535               // grid y
#define RS_U 8                          // i unroll

template <int J>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                              float* __restrict__ y, int T_in, int T_out, int o, int n,
                                                              int width, int K, int span, int ostr, int nq) {
  extern __shared__ float s_x[];
  const int row = blockIdx.y;
  const long long blk0 = (long long)blockIdx.x * span;
  const float* __restrict__ xr = x + (size_t)row * T_in;
  float* __restrict__ yr = y + (size_t)row * T_out;

  // staging: window sample p is xpad[blk0 o + p]; only addresses inside the row are dereferenced
  const int welems = (span - 1 + nq) * o;
  const long long s0 = blk0 * o - width;
  for (int p = threadIdx.x; p < welems; p += RS_THREADS) {
    const long long s = s0 + p;
    s_x[(p / o) * ostr + p % o] = (s >= 0 && s < T_in) ? xr[s] : 0.0f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lrow = lane < span ? lane : span - 1;          // lanes past the span read staged data, store nothing
  const long long blk = blk0 + lane;
  const int ngroups = (n + J - 1) / J;
  for (int g = wave; g < ngroups; g += RS_THREADS / 64) {
    const int j0 = g * J;
    const float* __restrict__ tp[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) tp[jj] = taps + (size_t)(j0 + jj < n ? j0 + jj : n - 1) * K;
    float acc[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) acc[jj] = 0.0f;
    for (int q = 0; q < nq; ++q) {
      const float* xs = s_x + (lrow + q) * ostr;
      const int ib = q * o;
      const int rend = K - ib < o ? K - ib : o;
      int r = 0;
      for (; r + RS_U <= rend; r += RS_U) {
        float xv[RS_U];
#pragma unroll
        for (int u = 0; u < RS_U; ++u) xv[u] = xs[r + u];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
          const float* t = tp[jj] + ib + r;
#pragma unroll
          for (int u = 0; u < RS_U; ++u) acc[jj] = fmaf(xv[u], t[u], acc[jj]);
        }
      }
      for (; r < rend; ++r) {
        const float xv = xs[r];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) acc[jj] = fmaf(xv, tp[jj][ib + r], acc[jj]);
      }
    }
    if (lane < span) {
#pragma unroll
      for (int jj = 0; jj < J; ++jj) {
        const long long out = blk * n + j0 + jj;
        if (j0 + jj < n && out < T_out) yr[out] = acc[jj];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
static long long rs_gcd(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// Modified Bessel function of the first kind, order 0 (torch.i0), by its power series sum_k ((x/2)^k / k!)^2.
static double rs_i0(double x) {
  const double h = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; ++k) {
    term *= h / ((double)k * k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

struct RsPlan {
  int o, n, width, K;
  double base;
};

static int rs_plan(int orig, int new_, int lowpass_filter_width, double rolloff, int method, double beta, RsPlan* p) {
  if (orig <= 0 || new_ <= 0 || lowpass_filter_width <= 0) return IAS_ERR_ARG;
  if (!(rolloff > 0.0 && rolloff <= 1.0)) return IAS_ERR_ARG;
  if (method != 0 && method != 1) return IAS_ERR_ARG;
  if (method == 1 && !(fabs(beta) <= 500.0)) return IAS_ERR_ARG;   // I0(beta) stays finite in fp64
  const long long g = rs_gcd(orig, new_);
  p->o = (int)(orig / g);
  p->n = (int)(new_ / g);
  p->base = (p->o < p->n ? p->o : p->n) * rolloff;
  const double w = ceil((double)lowpass_filter_width * p->o / p->base);
  if (!(w <= (double)(INT_MAX / 4))) return IAS_ERR_UNSUPPORTED;
  p->width = (int)w;
  const long long K = 2LL * p->width + p->o;
  if (K > INT_MAX || (long long)p->n * K > RS_TAP_CAP) return IAS_ERR_UNSUPPORTED;
  p->K = (int)K;
  return IAS_OK;
}

// Output blocks per workgroup for a shape, or 0 when one block's window (nq rows of ostr floats) does not fit the LDS.
static int rs_span(int o, int K, long long nblk) {
  const long long ostr = o | 1, nq = (K + o - 1) / o;
  long long span = RS_LDS_FLOATS / ostr - nq + 1;
  if (span < 1) return 0;
  if (span > RS_SPAN) span = RS_SPAN;
  if (span > nblk) span = nblk;
  return (int)span;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ias_resample_plan(int orig, int new_, int lowpass_filter_width, double rolloff, int method, double beta,
                                 int* plan) {
  if (!plan) return IAS_ERR_ARG;
  RsPlan p;
  const int st = rs_plan(orig, new_, lowpass_filter_width, rolloff, method, beta, &p);
  if (st != IAS_OK) return st;
  plan[0] = p.o;
  plan[1] = p.n;
  plan[2] = p.width;
  plan[3] = p.K;
  return IAS_OK;
}

extern "C" int ias_resample_build_taps(int orig, int new_, int lowpass_filter_width, double rolloff, int method,
                                       double beta, float* taps_host) {
  if (!taps_host) return IAS_ERR_ARG;
  RsPlan p;
  const int st = rs_plan(orig, new_, lowpass_filter_width, rolloff, method, beta, &p);
  if (st != IAS_OK) return st;
  const double lw = (double)lowpass_filter_width, scale = p.base / p.o;
  const double i0b = method == 1 ? rs_i0(beta) : 1.0;
  for (int j = 0; j < p.n; ++j) {
    for (int i = 0; i < p.K; ++i) {
      double t = ((double)(i - p.width) / p.o - (double)j / p.n) * p.base;
      t = t < -lw ? -lw : (t > lw ? lw : t);
      double win;
      if (method == 0) {
        const double c = cos(t * M_PI / lw / 2.0);
        win = c * c;
      } else {
        const double r = t / lw;
        win = rs_i0(beta * sqrt(1.0 - r * r)) / i0b;
      }
      t *= M_PI;
      const double k = t == 0.0 ? 1.0 : sin(t) / t;
      taps_host[(size_t)j * p.K + i] = (float)(k * (win * scale));
    }
  }
  return IAS_OK;
}

extern "C" long long ias_resample_out_len(long long T_in, int o, int n) {
  if (T_in < 1 || o < 1 || n < 1) return IAS_ERR_ARG;
  if (T_in > (LLONG_MAX - o) / n) return IAS_ERR_ARG;
  return ((long long)n * T_in + o - 1) / o;
}

extern "C" int ias_resample(const float* x, const float* taps, float* y, int B, int T_in, int o, int n, int width, int K,
                            void* stream_) {
  if (!x || !y || B < 1 || T_in < 1 || o < 1 || n < 1 || width < 0) return IAS_ERR_ARG;
  if ((long long)K != 2LL * width + o) return IAS_ERR_ARG;
  if ((long long)n * K > RS_TAP_CAP) return IAS_ERR_UNSUPPORTED;
  if (B > RS_MAX_ROWS) return IAS_ERR_UNSUPPORTED;
  const long long T_out = ias_resample_out_len(T_in, o, n);
  if (T_out < 1 || T_out > INT_MAX) return IAS_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  if (o == n) {                                              // the identity: a copy
    if (hipMemcpyAsync(y, x, (size_t)B * T_in * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
      return IAS_ERR_LAUNCH;
    return IAS_OK;
  }
  if (!taps) return IAS_ERR_ARG;
  const long long nblk = (T_out + n - 1) / n;
  const int span = rs_span(o, K, nblk);
  if (span < 1) return IAS_ERR_UNSUPPORTED;
  const int ostr = o | 1, nq = (K + o - 1) / o;
  const long long nspans = (nblk + span - 1) / span;
  if (nspans > INT_MAX) return IAS_ERR_UNSUPPORTED;
  const size_t lds = (size_t)(span - 1 + nq) * ostr * sizeof(float);
  const dim3 grid((unsigned)nspans, (unsigned)B), block(RS_THREADS);
  const int To = (int)T_out;
  if (n >= 8)
    hipLaunchKernelGGL(resample_kernel<8>, grid, block, lds, stream, x, taps, y, T_in, To, o, n, width, K, span, ostr, nq);
  else if (n >= 4)
    hipLaunchKernelGGL(resample_kernel<4>, grid, block, lds, stream, x, taps, y, T_in, To, o, n, width, K, span, ostr, nq);
  else if (n >= 2)
    hipLaunchKernelGGL(resample_kernel<2>, grid, block, lds, stream, x, taps, y, T_in, To, o, n, width, K, span, ostr, nq);
  else
    hipLaunchKernelGGL(resample_kernel<1>, grid, block, lds, stream, x, taps, y, T_in, To, o, n, width, K, span, ostr, nq);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
