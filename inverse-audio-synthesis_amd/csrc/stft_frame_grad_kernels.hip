// Frame part of the spectral losses' backward on the forward's wave-per-frame FFT core: stft_grad_wave_kernel,
// stft_grad2k_kernel, stft_grad512_kernel, their launcher and C entries.  (The overlap-add, combine and first-version
// kernels are in spectral_grad_kernels.hip, the forward in spectral_kernels.hip, what both use in stft_core.h.)
#include "ias_common.h"
#include <cstdlib>
#include "stft_core.h"

// Backward of the linear-bin losses, frame part, on the same wave-per-frame FFT core (round 2).
//
// d loss / d x_f for  loss_mode 1: scale * sum |V - t|  and  loss_mode 2: one MR-STFT resolution (cotangent
// gO = coef[0] (V - t) + coef[1] sign(V - t) / V), V = |X|^2 (power 2) or sqrt(|X|^2) (power 1; loss_mode 2 clamps at
// eps), linear bins (n_out = N/2 + 1).  The first version (csrc/spectral_grad_kernels.hip: one workgroup per frame
// pair, Stockham radix-4 with a workgroup barrier per stage) was 51 % of the configs[4] gradient step.  Here a wave
// owns a frame end to end:
//   forward   the stft_kernel passes (window, packed real FFT of N/2 complex points), unpack to X[k], X[N/2-k] in registers
//   adjoint   G[k] = 2 gP[k] X[k] per bin, in registers (a lane owns bins k and N/2 - k)
//   inverse   y[n] = Re sum_{k<=N/2} G[k] e^{+2 pi i k n / N} as ONE N/2-point complex inverse FFT:
//             with a[k] = G[k], a[0] = G[0] + G[N/2];  b[k] = G[k] e^{+2 pi i k / N}, b[0] = G[0] - G[N/2]:
//             y[2m] + i y[2m+1] = IDFT(Zin)[m],  Zin[k] = (a[k] + conj a[N/2-k]) / 2 + i (b[k] + conj b[N/2-k]) / 2;
//             the inverse transform is the same three passes on conj(Zin), conjugated again at the end
//   output    frame_grad[f][n] = window[n] y[n]  (the overlap-add stays in stft_grad_ola_kernel)
struct SgwArgs {
  const float* audio; const float* tables; const float* target; const double* coef; float* frame_grad;
  const int* mel_start; const int* mel_count; const int* mel_woff; const float* mel_w;   // MEL: the forward's CSR filters
  int T, F, hop, groups, power2, loss_mode, n_out, mel_nnz;
  float scale, eps;
  int G, cper, L, nchunks;   // SPAN kernels: frames per chunk, chunks per row, floats per chunk span, B * cper
};

// ---- the bin maths the kernels share.  Each helper stands where it left the instruction stream of its callers as it
// was (scripts/isa_diff.py); DESIGN.md section 4.5 lists the blocks that stayed a copy per kernel because it did not.
// The loss of one bin: value V of a bin from its power; d loss / d V from value and target (linear bins);
// d loss / d |X|^2 from d loss / d V.  c0, c1: the MR-STFT coefficient pair (loss_mode 2), the kernel's own variables,
// which CROW kernels reload at every chunk.  The members are references and the methods plain inline functions: that is
// the closure the kernels' lambdas were, and what keeps their code; copies of the four scalars let the compiler unswitch
// the frame loop on loss_mode (17 of the 22 kernels then change, up to ten VGPRs).
struct BinLoss {
  const SgwArgs& a;      // power2, loss_mode, eps, scale
  const float& c0;
  const float& c1;
  __device__ float value(float p) const {
    return a.power2 ? p : __builtin_amdgcn_sqrtf(a.loss_mode == 2 ? fmaxf(p, a.eps) : p);   // v_sqrt_f32
  }
  __device__ float value_grad(float v, float t) const {
    const float d = v - t;
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    return a.loss_mode == 2 ? c0 * d + c1 * sg * __builtin_amdgcn_rcpf(v) : sg * a.scale;   // v_rcp_f32 (1 ulp)
  }
  __device__ float power_grad(float gv, float v) const {
    if (a.power2) return gv;
    const bool live = a.loss_mode == 2 ? v > __builtin_amdgcn_sqrtf(a.eps) : v > 0.0f;   // a clamped (or zero) bin passes nothing
    return live ? 0.5f * gv * __builtin_amdgcn_rcpf(v) : 0.0f;
  }
};
// Unpack of the packed real FFT for the bin pair (k, N2 - k): Z[k], Z[N2 - k], w = W_N^k = e^{-2 pi i k / N} -> X[k], X[N2 - k]
__device__ __forceinline__ void bin_pair_unpack(cpx zk, cpx zn, cpx w, cpx& xk, cpx& xq) {
  const cpx ze = cmk(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
  const cpx zo = cmk(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
  const cpx t = cmul(w, zo);                                // W_N^k Zo[k]
  xk = cadd(ze, t);                                         // X[k]
  xq = cmk(ze.x - t.x, -(ze.y - t.y));                      // X[N2 - k] = conj(ze - t)
}
// Its adjoint for 0 < k < N2 / 2: ck = G[k], cq = G[N2 - k], w -> the pair's inverse inputs Zin[k], Zin[N2 - k].  (The edge
// pair k = 0 -- real X, Zin[0] = a[0] + i b[0] with a[0] = G[0] + G[N2], b[0] = G[0] - G[N2] -- is one line in the caller:
// taken in here behind a flag, stft_grad2k_kernel's SPAN forms came out in another instruction order.)
__device__ __forceinline__ void bin_pair_adjoint(cpx ck, cpx cq, cpx w, cpx& zk_in, cpx& zn_in) {
  const cpx bk = cmul(ck, cmk(w.x, -w.y));                  // b[k] = G[k] e^{+2 pi i k / N}
  const cpx bn = cmul(cq, cmk(-w.x, -w.y));                 // b[N2 - k] = G[N2 - k] (-W^k)
  // Zin[k] = (a[k] + conj a[kn]) / 2 + i (b[k] + conj b[kn]) / 2, and the same with k <-> kn
  const cpx ak = cmk(0.5f * (ck.x + cq.x), 0.5f * (ck.y - cq.y));
  const cpx sk = cmk(0.5f * (bk.x + bn.x), 0.5f * (bk.y - bn.y));
  zk_in = cmk(ak.x - sk.y, ak.y + sk.x);                    // Zin[k]
  zn_in = cmk(ak.x + sk.y, -ak.y + sk.x);                   // Zin[N2 - k] = conj(ak) + i conj(sk)
}

// MEL: the loss is taken on O = melW^T V (loss_mode 1 only).  V goes to LDS, a lane computes two outputs with the
// forward's padded filter loops, their cotangents are scattered back to the bins with LDS float atomics (a bin lies under
// at most two triangular filters: the sum of two terms does not depend on their order), then the bins continue as above.
//
// SPAN (round 3): overlap-add inside the kernel.  A wave owns a CHUNK of G consecutive frames of one row and walks it
// in order; the windowed frame gradients are added into a ring of n_fft floats in LDS (one wave, program order: the
// sum over frames is in frame order, deterministic), and after every frame the hop samples no later frame of the chunk
// touches leave the ring for the chunk's span  frame_grad[chunk][L], L = (G - 1) hop + n_fft.  The [B,F,n_fft] tensor
// (8.5 - 10 floats per audio sample, written here and read again by stft_grad_ola_kernel) shrinks to ~1.2 - 1.5
// floats per sample; stft_grad_combine_kernel adds the two chunks that meet at a sample, lower chunk first.
//
// CROW (loss_mode 2 only): coef holds one pair per row, [B][2] (the per-sound MR-STFT losses, ias_stft_grad_spans_mrstft_rows);
// a wave reads the pair of the row it is working on at the start of every chunk (a SPAN wave can walk chunks of several
// rows).  A row whose pair is {0, 0} gets exactly 0.
template <int LOG2N, bool MEL, bool SPAN, bool CROW>
__global__ __launch_bounds__(256) void stft_grad_wave_kernel(const SgwArgs a) {
  constexpr int SP_WAVES = 4, SP_THREADS = 256;
  constexpr int NFFT = 1 << LOG2N, N2 = NFFT / 2, R = N2 / 64, NPAIR = 8 * R, NP_IT = (NPAIR + 63) / 64;
  constexpr int SCR = NPAIR * IAS_S2_ROW, NUNP = (N2 / 2) / 64 + 1, NB = N2 + 1;
  constexpr int NTAB = 64 * (2 * R + 2 * R + 16 * NP_IT + 2 * NUNP);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cpx* s_scr = reinterpret_cast<cpx*>(smem);
  float* s_ring = reinterpret_cast<float*>(s_scr + SP_WAVES * SCR);          // SPAN: [wave][NFFT]
  // the tables are an LDS object of their own: carved out of the array that holds the scratch, every table read behind a
  // scratch store was ordered after it (see stft2_kernel)
  __shared__ cpx s_tab[NTAB / 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (SPAN) for (int i = tid; i < SP_WAVES * NFFT; i += SP_THREADS) s_ring[i] = 0.0f;
  for (int i = tid; i < NTAB / 2; i += SP_THREADS) {
    const int pp = i >> 6, l = i & 63;
    s_tab[i] = cmk(a.tables[64 * (2 * pp) + l], a.tables[64 * (2 * pp + 1) + l]);
  }
  // MEL: padded weights + descriptors (as in stft_kernel), then per wave the output cotangents and the bin cotangents
  float* s_melw = reinterpret_cast<float*>(s_scr + SP_WAVES * SCR + (SPAN ? SP_WAVES * N2 : 0));
  const int melw_words = MEL ? mel_padded_words(a.mel_nnz, a.n_out) : 0;
  int* s_meli = reinterpret_cast<int*>(s_melw + melw_words);            // [3][n_out]: start, padded count, padded offset
  const int so_words = MEL ? ((a.n_out + 3) & ~3) : 0;
  float* s_go = reinterpret_cast<float*>(s_meli + (MEL ? ((3 * a.n_out + 3) & ~3) : 0)) + wave * (so_words + NB + 7);
  float* s_gv = s_go + so_words;                                        // [NB + 4] (+ slack for the zero padding)
  if (MEL) {
    for (int i = tid; i < melw_words; i += SP_THREADS) s_melw[i] = 0.0f;
    for (int i = tid; i < a.n_out; i += SP_THREADS) {
      s_meli[i] = a.mel_start[i];
      s_meli[a.n_out + i] = (a.mel_count[i] + 3) & ~3;
    }
    __syncthreads();
    for (int i = tid; i < a.n_out; i += SP_THREADS) {
      int off = 0;
      for (int m = 0; m < i; ++m) off += s_meli[a.n_out + m];
      s_meli[2 * a.n_out + i] = off;
    }
    __syncthreads();
    for (int i = tid; i < a.n_out; i += SP_THREADS) {
      const int n = a.mel_count[i], src = a.mel_woff[i], dst = s_meli[2 * a.n_out + i];
      for (int j = 0; j < n; ++j) s_melw[dst + j] = a.mel_w[src + j];
    }
  }
  const cpx* t_win = s_tab + lane;
  const cpx* t_tw1 = t_win + 64 * R;
  const cpx* t_tw2 = t_tw1 + 64 * R;
  const cpx* t_twu = t_tw2 + 64 * 8 * NP_IT;
  // the padded filter loop reads up to three words past the NB values V of the wave's scratch: zeroed once, as in
  // stft_kernel (n_fft 512: words NB and NB + 1 .. 2 lie in the padding columns of row 12, which no pass writes)
  if (MEL && lane < 3) reinterpret_cast<float*>(s_scr + wave * SCR)[NB + lane] = 0.0f;
  __syncthreads();
  cpx* sA = s_scr + wave * SCR;
  float c0 = 0.0f, c1 = 0.0f;
  if constexpr (!CROW) { if (a.loss_mode == 2) { c0 = (float)a.coef[0]; c1 = (float)a.coef[1]; } }

  // the three passes of stft_kernel: v = the lane's R points (64 n1 + lane) -> DFT in natural order, sA[IAS_S2_UP(k)]
  auto fft = [&](cpx (&v)[R]) {
    dftR<R>(v);
    {
      const int c = lane & 7, aa = lane >> 3;
#pragma unroll
      for (int k1 = 0; k1 < R; ++k1) sA[(k1 * 8 + c) * IAS_S2_ROW + aa] = cmul(v[k1], t_tw1[64 * k1]);
    }
    wave_lds_sync();
    cpx u[NP_IT][8];
#pragma unroll
    for (int i = 0; i < NP_IT; ++i) {
      const int p = lane + 64 * i;
      if (p < NPAIR) {
#pragma unroll
        for (int q = 0; q < 8; ++q) u[i][q] = sA[p * IAS_S2_ROW + q];
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < NP_IT; ++i) {
      const int p = lane + 64 * i;
      if (p < NPAIR) {
        const int k1 = p >> 3, c = p & 7;
        dft8(u[i]);
#pragma unroll
        for (int d = 0; d < 8; ++d) sA[(k1 * 8 + d) * IAS_S2_ROW + c] = cmul(u[i][d], t_tw2[64 * (8 * i + d)]);
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < NP_IT; ++i) {
      const int p = lane + 64 * i;
      if (p < NPAIR) {
#pragma unroll
        for (int q = 0; q < 8; ++q) u[i][q] = sA[p * IAS_S2_ROW + q];
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < NP_IT; ++i) {
      const int p = lane + 64 * i;
      if (p < NPAIR) {
        const int k1 = p >> 3, d = p & 7;
        dft8(u[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const int k = k1 + R * d + 8 * R * e; sA[IAS_S2_UP(k)] = u[i][e]; }
      }
    }
    wave_lds_sync();
  };
  const BinLoss bl = {a, c0, c1};   // (constructed here, behind the transform's lambda: see BinLoss)

  float xc[2 * R];
  float* ring = s_ring + wave * NFFT;
  const int cstep = SPAN ? (int)gridDim.x * SP_WAVES : 1;
  for (int c = SPAN ? (int)blockIdx.x * SP_WAVES + wave : 0; c < (SPAN ? a.nchunks : 1); c += cstep) {
  int b, f_lo, f_hi;
  if (SPAN) { b = c / a.cper; f_lo = (c - b * a.cper) * a.G; f_hi = min(f_lo + a.G, a.F); }
  else { b = blockIdx.y; f_lo = blockIdx.x * a.groups + wave; f_hi = min((int)blockIdx.x * a.groups + a.groups, a.F); }
  if constexpr (CROW) { c0 = (float)a.coef[2 * (size_t)b]; c1 = (float)a.coef[2 * (size_t)b + 1]; }
  const float* arow = a.audio + (size_t)b * a.T;
  float* span = a.frame_grad + (size_t)c * a.L;
  for (int f = f_lo; f < f_hi; f += SPAN ? 1 : SP_WAVES) {
    load_frame<R, N2>(arow, a.T, a.hop, f, lane, xc);
    const float* trow = a.target + ((size_t)b * a.F + f) * (MEL ? a.n_out : NB);
    // linear bins: the lane's target values are requested with the frame and consumed after the forward transform
    float tk_[NUNP], tq_[NUNP];
    if (!MEL) {
#pragma unroll
      for (int i = 0; i < NUNP; ++i) {
        const int k = lane + 64 * i;
        tk_[i] = tq_[i] = 0.0f;
        if (k <= N2 / 2) { tk_[i] = trow[k]; tq_[i] = trow[N2 - k]; }
      }
    }
    cpx v[R];
#pragma unroll
    for (int n1 = 0; n1 < R; ++n1) v[n1] = cmk(xc[2 * n1], xc[2 * n1 + 1]) * t_win[64 * n1];
    fft(v);
    // unpack per bin pair (k, N2 - k), k = lane + 64 i <= N2 / 2: X and V of both bins in registers
    cpx xk_[NUNP], xq_[NUNP];
    float vk_[NUNP], vq_[NUNP], gk_[NUNP], gq_[NUNP];
#pragma unroll
    for (int i = 0; i < NUNP; ++i) {
      const int k = lane + 64 * i;
      xk_[i] = xq_[i] = cmk(0.0f, 0.0f);
      vk_[i] = vq_[i] = gk_[i] = gq_[i] = 0.0f;
      if (k <= N2 / 2) {
        const int kn = (N2 - k) & (N2 - 1);
        const cpx zk = sA[IAS_S2_UP(k)], zn = sA[IAS_S2_UP(kn)];
        const cpx ze = cmk(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
        const cpx zo = cmk(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
        const cpx t = cmul(t_twu[64 * i], zo);            // W_N^k Zo[k]
        xk_[i] = cadd(ze, t);                             // X[k]
        xq_[i] = cmk(ze.x - t.x, -(ze.y - t.y));          // X[N2 - k]
        vk_[i] = bl.value(xk_[i].x * xk_[i].x + xk_[i].y * xk_[i].y);
        vq_[i] = bl.value(xq_[i].x * xq_[i].x + xq_[i].y * xq_[i].y);
        if (!MEL) { gk_[i] = bl.value_grad(vk_[i], tk_[i]); gq_[i] = bl.value_grad(vq_[i], tq_[i]); }
      }
    }
    if (MEL) {
      wave_lds_sync();                                    // every Z read is done: V overwrites the scratch
      float* P = reinterpret_cast<float*>(sA);
#pragma unroll
      for (int i = 0; i < NUNP; ++i) {
        const int k = lane + 64 * i;
        if (k <= N2 / 2) { P[k] = vk_[i]; P[N2 - k] = vq_[i]; }
      }
      for (int i = lane; i < NB + 4; i += 64) s_gv[i] = 0.0f;
      wave_lds_sync();
      for (int m0 = 0; m0 < a.n_out; m0 += 64) {
        const int m = m0 + lane;
        if (m < a.n_out) {
          const int s0 = s_meli[m], n4 = s_meli[a.n_out + m];
          const float* w = s_melw + s_meli[2 * a.n_out + m];
          float o = 0.0f;
          for (int j = 0; j < n4; j += 4) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + j);
            const float* pp = P + s0 + j;
            o = fmaf(wv[3], pp[3], fmaf(wv[2], pp[2], fmaf(wv[1], pp[1], fmaf(wv[0], pp[0], o))));
          }
          s_go[m] = bl.value_grad(o, trow[m]);
        }
      }
      wave_lds_sync();
      for (int m0 = 0; m0 < a.n_out; m0 += 64) {
        const int m = m0 + lane;
        if (m < a.n_out) {
          const int s0 = s_meli[m], n4 = s_meli[a.n_out + m];
          const float* w = s_melw + s_meli[2 * a.n_out + m];
          const float go = s_go[m];
          for (int j = 0; j < n4; ++j) {
            const float wj = w[j];
            if (wj != 0.0f) atomicAdd(&s_gv[s0 + j], wj * go);
          }
        }
      }
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < NUNP; ++i) {
        const int k = lane + 64 * i;
        if (k <= N2 / 2) { gk_[i] = s_gv[k]; gq_[i] = s_gv[N2 - k]; }
      }
    }
    // adjoint per bin pair; the inverse input in registers
    cpx zk_in[NUNP], zn_in[NUNP];
#pragma unroll
    for (int i = 0; i < NUNP; ++i) {
      const int k = lane + 64 * i;
      zk_in[i] = zn_in[i] = cmk(0.0f, 0.0f);
      if (k <= N2 / 2) {
        const cpx w = t_twu[64 * i];                      // W_N^k = e^{-2 pi i k / N}
        const cpx ck = xk_[i] * (2.0f * bl.power_grad(gk_[i], vk_[i]));   // G[k]
        const cpx cq = xq_[i] * (2.0f * bl.power_grad(gq_[i], vq_[i]));   // G[N2 - k]
        if (k == 0) {
          // edge bins (real X): a[0] = G[0] + G[N2], b[0] = G[0] - G[N2]; Zin[0] = a[0] + i b[0]
          zk_in[i] = cmk(ck.x + cq.x, ck.x - cq.x);
          zn_in[i] = zk_in[i];
        } else {
          const cpx wc = cmk(w.x, -w.y);                  // e^{+2 pi i k / N}
          const cpx bk = cmul(ck, wc);                    // b[k]
          const cpx bn = cmul(cq, cmk(-w.x, -w.y));       // b[N2 - k] = G[N2 - k] (-W^k)
          // Zin[k] = (a[k] + conj a[kn]) / 2 + i (b[k] + conj b[kn]) / 2, and the same with k <-> kn
          const cpx ak = cmk(0.5f * (ck.x + cq.x), 0.5f * (ck.y - cq.y)), an = cmk(ak.x, -ak.y);
          const cpx sk = cmk(0.5f * (bk.x + bn.x), 0.5f * (bk.y - bn.y)), sn = cmk(sk.x, -sk.y);
          zk_in[i] = cmk(ak.x - sk.y, ak.y + sk.x);
          zn_in[i] = cmk(an.x - sn.y, an.y + sn.x);
        }
      }
    }
    wave_lds_sync();                                      // every Z read is done
    // conj(Zin) in natural order (padded like Z), then the lane's R points of it
#pragma unroll
    for (int i = 0; i < NUNP; ++i) {
      const int k = lane + 64 * i;
      if (k <= N2 / 2) {
        const int kn = (N2 - k) & (N2 - 1);
        sA[IAS_S2_UP(k)] = cmk(zk_in[i].x, -zk_in[i].y);
        if (kn != k) sA[IAS_S2_UP(kn)] = cmk(zn_in[i].x, -zn_in[i].y);
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int n1 = 0; n1 < R; ++n1) { const int p = 64 * n1 + lane; v[n1] = sA[IAS_S2_UP(p)]; }
    wave_lds_sync();
    fft(v);
    // z[m] = conj(out[m]) = y[2m] + i y[2m+1];  frame_grad = window * y
    if (SPAN) {
      const int rb = ((f - f_lo) * a.hop) & (NFFT - 1);     // ring position of the frame's first sample (hop is even)
#pragma unroll
      for (int n1 = 0; n1 < R; ++n1) {
        const int m = 64 * n1 + lane;
        const cpx o = sA[IAS_S2_UP(m)];
        const cpx w2 = t_win[64 * n1];
        cpx* rp = reinterpret_cast<cpx*>(ring + ((rb + 2 * m) & (NFFT - 1)));
        const cpx cur = *rp;
        *rp = cmk(cur.x + w2.x * o.x, cur.y - w2.y * o.y);
      }
      wave_lds_sync();
      float* sp = span + (size_t)(f - f_lo) * a.hop;         // the hop samples no later frame of the chunk reaches
      for (int i = lane; i < a.hop; i += 64) {
        const int idx = (rb + i) & (NFFT - 1);
        sp[i] = ring[idx];
        ring[idx] = 0.0f;
      }
      wave_lds_sync();
    } else {
      float* out = a.frame_grad + ((size_t)b * a.F + f) * NFFT;
#pragma unroll
      for (int n1 = 0; n1 < R; ++n1) {
        const int m = 64 * n1 + lane;
        const cpx o = sA[IAS_S2_UP(m)];
        const cpx w2 = t_win[64 * n1];
        *reinterpret_cast<cpx*>(out + 2 * m) = cmk(w2.x * o.x, -w2.y * o.y);
      }
      wave_lds_sync();
    }
  }
  if (SPAN && f_hi > f_lo) {                                 // the chunk's tail: what is left in the ring
    const int nf = f_hi - f_lo, rb = (nf * a.hop) & (NFFT - 1);
    float* sp = span + (size_t)nf * a.hop;
    for (int i = lane; i < NFFT - a.hop; i += 64) {
      const int idx = (rb + i) & (NFFT - 1);
      sp[i] = ring[idx];
      ring[idx] = 0.0f;
    }
    wave_lds_sync();
  }
  }
}

// Backward of the linear-bin losses for n_fft 2048 on the 8-points-per-lane core (round 3): the forward of
// stft2_kernel<.., NSUB = 2> (two 512-point half-transforms, in-lane combine, half-spectrum unpack), the cotangent per
// bin pair in registers, then the inverse 1024-point transform split the other way round (decimation in frequency):
//     A_p[k] = (Zin[k] + (-1)^p Zin[k + 512]) e^{+2 pi i k p / 1024},   z[2m + p] = IDFT_512(A_p)[m],   p = 0, 1,
// Zin[k + 512] reaches the lane that owns k through one LDS exchange (it is computed as the partner value of bin 512 - k),
// each IDFT_512 runs as the three forward passes on the conjugate, and a lane ends up with the four samples 4m .. 4m+3
// of its m = k1 + 8 d + 64 e: one 16-byte store per (lane, e).  Same arithmetic as stft_grad_wave_kernel<11, false>,
// which needs 198 VGPRs and 9.2 KB of scratch per wave (2 waves per SIMD) for its radix-16 first pass.
//
// SPAN: as in stft_grad_wave_kernel (a wave walks a chunk of G consecutive frames, overlap-add in an LDS ring, hop % 4
// == 0).  The ring is kept in 16-byte units q = sample / 4 at slot q ^ ((q >> 3) & 7): the lanes' units m = k1 + 8 d
// (+ 64 e) are 8 apart for consecutive lanes, the swizzle spreads them over the banks.
// CROW: per-row coefficient pairs, as in stft_grad_wave_kernel (read for every chunk or frame: both walk across rows).
template <int SP_WAVES, bool SPAN, bool CROW>
__global__ __launch_bounds__(64 * SP_WAVES, SPAN ? 2 : 3 * SP_WAVES / 8) void stft_grad2k_kernel(const SgwArgs a, int nframes, unsigned magicF) {
  constexpr int SP_THREADS = 64 * SP_WAVES, N2 = 1024, HALF = 512, NFFT = 2048, SCR = 64 * IAS_S2_ROW, NB = N2 + 1;
  constexpr int NTAB = 16 + 8 + 8 + 8 + 8 + 16;   // stft2's 2048 section + the window at the lane's OUTPUT samples
  constexpr int V2_BASE_2048 = 32 + 32 + 32 + 18;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cpx* s_scr = reinterpret_cast<cpx*>(smem);
  f32x4* s_ring = reinterpret_cast<f32x4*>(s_scr + SP_WAVES * SCR);         // SPAN: [wave][NFFT / 4]
  __shared__ cpx s_tab[NTAB * 64];                                          // an LDS object of its own (see stft2_kernel)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (SPAN) for (int i = tid; i < SP_WAVES * NFFT / 4; i += SP_THREADS) s_ring[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  for (int i = tid; i < NTAB * 64; i += SP_THREADS) {
    const int pp = i >> 6, l = i & 63, src = V2_BASE_2048 + 2 * pp;
    s_tab[i] = cmk(a.tables[64 * src + l], a.tables[64 * (src + 1) + l]);
  }
  const cpx* t_win = s_tab + lane;              // [8 sub + n1]
  const cpx* t_tw1 = t_win + 64 * 16;
  const cpx* t_tw2 = t_tw1 + 64 * 8;
  const cpx* t_cmb = t_tw2 + 64 * 8;            // [e] -> W_1024^k
  const cpx* t_twu = t_cmb + 64 * 8;            // [e] -> W_2048^k
  const cpx* t_wo = t_twu + 64 * 8;             // [2 e + h] -> window at samples 4 m + 2 h + {0, 1}, m = k1 + 8 d + 64 e
  __syncthreads();
  cpx* sA = s_scr + wave * SCR;
  const int k1 = lane >> 3, dd = lane & 7, kl = k1 + 8 * dd;
  float c0 = 0.0f, c1 = 0.0f;
  if constexpr (!CROW) { if (a.loss_mode == 2) { c0 = (float)a.coef[0]; c1 = (float)a.coef[1]; } }
  const BinLoss bl = {a, c0, c1};   // (constructed here, behind the transform's lambda: see BinLoss)
  auto pad = [](int i) { return IAS_S2_UP(i); };   // i < 512: two pad elements per eight (see IAS_S2_ROW)
  // the three radix-8 passes of a 512-point transform: v = the lane's points 64 n1 + lane -> u[e] at kl + 64 e
  auto fft512 = [&](cpx (&v)[8], cpx (&u)[8]) {
    dft8(v);
    {
      const int c = lane & 7, aa = lane >> 3;
#pragma unroll
      for (int q = 0; q < 8; ++q) sA[(q * 8 + c) * IAS_S2_ROW + aa] = cmul(v[q], t_tw1[64 * q]);
    }
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) u[q] = sA[lane * IAS_S2_ROW + q];
    wave_lds_sync();
    dft8(u);
#pragma unroll
    for (int d = 0; d < 8; ++d) sA[(k1 * 8 + d) * IAS_S2_ROW + dd] = cmul(u[d], t_tw2[64 * d]);
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) u[q] = sA[lane * IAS_S2_ROW + q];
    wave_lds_sync();
    dft8(u);
  };

  const int gw = blockIdx.x * SP_WAVES + wave, nw = gridDim.x * SP_WAVES;
  f32x4* ring = s_ring + wave * (NFFT / 4);
  auto slot = [](int q) { return q ^ ((q >> 3) & 7); };
  for (int c = gw; c < (SPAN ? a.nchunks : nframes); c += nw) {
  int b, f_lo, f_hi;
  if (SPAN) { b = c / a.cper; f_lo = (c - b * a.cper) * a.G; f_hi = min(f_lo + a.G, a.F); }
  else {
    unsigned q0 = __umulhi((unsigned)c, magicF);
    int fr0 = c - (int)q0 * a.F;
    if (fr0 >= a.F) { fr0 -= a.F; ++q0; }
    b = (int)q0; f_lo = fr0; f_hi = fr0 + 1;
  }
  if constexpr (CROW) { c0 = (float)a.coef[2 * (size_t)b]; c1 = (float)a.coef[2 * (size_t)b + 1]; }
  f32x4* span = reinterpret_cast<f32x4*>(a.frame_grad + (size_t)c * a.L);   // SPAN (L % 4 == 0)
  for (int fr = f_lo; fr < f_hi; ++fr) {
    const int fi = b * a.F + fr;
    float xc[32];
    stft2_load_frame<2>(a.audio + (size_t)b * a.T, a.T, a.hop, fr, lane, xc);
    const float* trow = a.target + (size_t)fi * NB;
    // the lane's target values are requested with the frame and consumed after the forward transform
    float tk_[8], tq_[8], th_ = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { tk_[e] = trow[kl + 64 * e]; tq_[e] = trow[N2 - kl - 64 * e]; }
    if (lane == 0) th_ = trow[HALF];
    // ---- forward: Z[k], Z[k + 512] for k = kl + 64 e
    cpx zlo[8], zhi[8];
    {
      cpx ue[8], u[8], v[8];
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) v[n1] = cmk(xc[2 * n1], xc[2 * n1 + 1]) * t_win[64 * n1];
      fft512(v, ue);
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) v[n1] = cmk(xc[16 + 2 * n1], xc[16 + 2 * n1 + 1]) * t_win[64 * (8 + n1)];
      fft512(v, u);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const cpx t = cmul(u[e], t_cmb[64 * e]); zlo[e] = cadd(ue[e], t); zhi[e] = csub(ue[e], t); }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sA[pad(kl + 64 * e)] = zhi[e];
    wave_lds_sync();
    // ---- per bin pair (k, N2 - k): X, value, cotangent, the pair's two inverse inputs
    cpx zk_in[8], zn_in[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = kl + 64 * e;
      cpx zn = sA[pad((HALF - k) & (HALF - 1))];
      const cpx zk = zlo[e];
      if (e == 0 && k == 0) zn = zk;
      const cpx w = t_twu[64 * e];                              // W_N^k = e^{-2 pi i k / N}
      cpx xk, xq;
      bin_pair_unpack(zk, zn, w, xk, xq);
      const float vk = bl.value(xk.x * xk.x + xk.y * xk.y), vq = bl.value(xq.x * xq.x + xq.y * xq.y);
      const float gk = bl.value_grad(vk, tk_[e]), gq = bl.value_grad(vq, tq_[e]);
      const cpx ck = xk * (2.0f * bl.power_grad(gk, vk));          // G[k]
      const cpx cq = xq * (2.0f * bl.power_grad(gq, vq));          // G[N2 - k]
      if (e == 0 && k == 0) { zk_in[e] = cmk(ck.x + cq.x, ck.x - cq.x); zn_in[e] = zk_in[e]; }   // edge bins (real X): a[0] + i b[0]
      else bin_pair_adjoint(ck, cq, w, zk_in[e], zn_in[e]);
    }
    // bin HALF pairs with itself: X[HALF] = conj(Z[HALF]) (lane 0 holds Z[HALF] = zhi[0])
    cpx zh_in;
    {
      const cpx xh = cmk(zhi[0].x, -zhi[0].y);
      const float vh = bl.value(xh.x * xh.x + xh.y * xh.y);
      const float gh = bl.value_grad(vh, th_);
      const cpx ch = xh * (2.0f * bl.power_grad(gh, vh));
      zh_in = cmk(ch.x, -ch.y);                                 // (ch + conj ch)/2 + i (i ch + conj(i ch))/2 = conj(ch)
    }
    wave_lds_sync();                                            // every Z read is done
    // ---- Zin[k + 512] to the lane that owns k: it was computed as the partner value of bin 512 - k
#pragma unroll
    for (int e = 0; e < 8; ++e) { const int k = kl + 64 * e; if (k != 0) sA[pad(HALF - k)] = zn_in[e]; }
    if (lane == 0) sA[0] = zh_in;
    wave_lds_sync();
    cpx a0[8], a1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const cpx zu = sA[pad(kl + 64 * e)];
      const cpx wc = t_cmb[64 * e];                             // W_1024^k; its conjugate is e^{+2 pi i k / 1024}
      a0[e] = cadd(zk_in[e], zu);
      a1[e] = cmul(csub(zk_in[e], zu), cmk(wc.x, -wc.y));
    }
    wave_lds_sync();
    // ---- the two inverse half-transforms, as forward passes on the conjugate
    cpx r0[8], r1[8];
    {
      cpx v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) sA[pad(kl + 64 * e)] = cmk(a0[e].x, -a0[e].y);
      wave_lds_sync();
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) v[n1] = sA[pad(64 * n1 + lane)];
      wave_lds_sync();
      fft512(v, r0);
      wave_lds_sync();
#pragma unroll
      for (int e = 0; e < 8; ++e) sA[pad(kl + 64 * e)] = cmk(a1[e].x, -a1[e].y);
      wave_lds_sync();
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) v[n1] = sA[pad(64 * n1 + lane)];
      wave_lds_sync();
      fft512(v, r1);
      wave_lds_sync();
    }
    // ---- frame_grad: samples 4 m .. 4 m + 3 of m = kl + 64 e = (y[2(2m)], y[2(2m)+1], y[2(2m+1)], y[2(2m+1)+1]) x window
    if (SPAN) {
      const int h4 = a.hop >> 2, rb = ((fr - f_lo) * h4) & (NFFT / 4 - 1);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = kl + 64 * e;
        const cpx w0 = t_wo[64 * (2 * e)], w1 = t_wo[64 * (2 * e + 1)];
        f32x4* rp = ring + slot((rb + m) & (NFFT / 4 - 1));
        const f32x4 cur = *rp;
        *rp = (f32x4){cur[0] + w0.x * r0[e].x, cur[1] - w0.y * r0[e].y, cur[2] + w1.x * r1[e].x, cur[3] - w1.y * r1[e].y};
      }
      wave_lds_sync();
      f32x4* sp = span + (size_t)(fr - f_lo) * h4;
      for (int i = lane; i < h4; i += 64) {
        f32x4* rp = ring + slot((rb + i) & (NFFT / 4 - 1));
        sp[i] = *rp;
        *rp = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
      }
      wave_lds_sync();
    } else {
      float* out = a.frame_grad + (size_t)fi * NFFT;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = kl + 64 * e;
        const cpx w0 = t_wo[64 * (2 * e)], w1 = t_wo[64 * (2 * e + 1)];
        *reinterpret_cast<f32x4*>(out + 4 * m) = (f32x4){w0.x * r0[e].x, -w0.y * r0[e].y, w1.x * r1[e].x, -w1.y * r1[e].y};
      }
    }
  }
  if (SPAN && f_hi > f_lo) {                                 // the chunk's tail: what is left in the ring
    const int h4 = a.hop >> 2, nf = f_hi - f_lo, rb = (nf * h4) & (NFFT / 4 - 1);
    f32x4* sp = span + (size_t)nf * h4;
    for (int i = lane; i < NFFT / 4 - h4; i += 64) {
      f32x4* rp = ring + slot((rb + i) & (NFFT / 4 - 1));
      sp[i] = *rp;
      *rp = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    wave_lds_sync();
  }
  }
}

// Backward of the linear-bin losses for n_fft 512, two frames per wave (the lane layout of stft2h_kernel), overlap-add
// inside the kernel (SPAN form only: ias_stft_grad_spans).  A wave walks its chunk two consecutive frames at a time:
// forward transform of both, cotangents per bin pair in the lane that owns the pair (lanes 0..31 frame A, 32..63 frame
// B), the inverse inputs Zin of both frames through the scratch in natural order, ONE more run of the three passes on
// their conjugates, then frame A's lanes add their windowed samples into the ring, after them frame B's (frame order:
// deterministic), and the 2 hop samples no later frame reaches leave the ring.
// CROW: per-row coefficient pairs, as in stft_grad_wave_kernel.
template <int SP_WAVES, bool CROW>
__global__ __launch_bounds__(64 * SP_WAVES, SP_WAVES / 2) void stft_grad512_kernel(const SgwArgs a) {
  constexpr int SP_THREADS = 64 * SP_WAVES, SCR = 64 * IAS_S2_ROW, NFFT = 512, N2 = 256, HALF = 128, NB = 257;
  constexpr int NTAB = 4 + 4 + 8 + 4 + 8;    // stft2h's tables + the window at the lane's OUTPUT samples
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cpx* s_scr = reinterpret_cast<cpx*>(smem);
  float* s_ring = reinterpret_cast<float*>(s_scr + SP_WAVES * SCR);         // [wave][NFFT]
  __shared__ cpx s_tab[NTAB * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < SP_WAVES * NFFT; i += SP_THREADS) s_ring[i] = 0.0f;
  // n_fft 512 block of ias_stft_build_tables: [0,8) window, [8,16) pass 1, [16,32) pass 2, [38,46) unpack, [46,62) output window
  for (int i = tid; i < NTAB * 64; i += SP_THREADS) {
    const int pp = i >> 6, l = i & 63, src = pp < 16 ? 2 * pp : 38 + 2 * (pp - 16);
    s_tab[i] = cmk(a.tables[64 * src + l], a.tables[64 * (src + 1) + l]);
  }
  const cpx* t_win = s_tab + lane;
  const cpx* t_tw1 = t_win + 64 * 4;
  const cpx* t_tw2 = t_tw1 + 64 * 4;
  const cpx* t_twu = t_tw2 + 64 * 8;          // [e] -> W_512^k, k = kl + 32 e (e < 4)
  const cpx* t_wo = t_twu + 64 * 4;           // [e] -> window at samples 2 m, 2 m + 1, m = kl + 32 e (e < 8)
  __syncthreads();
  cpx* sA = s_scr + wave * SCR;
  float* ring = s_ring + wave * NFFT;
  const int slot = lane >> 3, dd = lane & 7, fr = lane >> 5, kl = (slot & 3) + 4 * dd;
  float c0 = 0.0f, c1 = 0.0f;
  if constexpr (!CROW) { if (a.loss_mode == 2) { c0 = (float)a.coef[0]; c1 = (float)a.coef[1]; } }
  const BinLoss bl = {a, c0, c1};   // (constructed here, behind the transform's lambda: see BinLoss)
  auto pad = [](int i) { return IAS_S2_UP(i); };   // i < 512: two pad elements per eight (see IAS_S2_ROW)
  // v[0..3] / v[4..7]: the lane's points 64 n1 + lane of frame A / B  ->  u[e] = transform of the lane's own frame
  // (slot >> 2) at kl + 32 e
  auto fft2 = [&](cpx (&v)[8], cpx (&u)[8]) {
    cpx (&va)[4] = reinterpret_cast<cpx (&)[4]>(v[0]);
    cpx (&vb)[4] = reinterpret_cast<cpx (&)[4]>(v[4]);
    dftR<4>(va); dftR<4>(vb);
    {
      const int c = lane & 7, aa = lane >> 3;
#pragma unroll
      for (int q = 0; q < 8; ++q) sA[(q * 8 + c) * IAS_S2_ROW + aa] = cmul(v[q], t_tw1[64 * (q & 3)]);
    }
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) u[q] = sA[lane * IAS_S2_ROW + q];
    wave_lds_sync();
    dft8(u);
#pragma unroll
    for (int d = 0; d < 8; ++d) sA[(slot * 8 + d) * IAS_S2_ROW + dd] = cmul(u[d], t_tw2[64 * d]);
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) u[q] = sA[lane * IAS_S2_ROW + q];
    wave_lds_sync();
    dft8(u);
  };

  const int cstep = (int)gridDim.x * SP_WAVES;
  for (int c = (int)blockIdx.x * SP_WAVES + wave; c < a.nchunks; c += cstep) {
    const int b = c / a.cper, f_lo = (c - b * a.cper) * a.G, f_hi = min(f_lo + a.G, a.F);
    if constexpr (CROW) { c0 = (float)a.coef[2 * (size_t)b]; c1 = (float)a.coef[2 * (size_t)b + 1]; }
    const float* arow = a.audio + (size_t)b * a.T;
    float* span = a.frame_grad + (size_t)c * a.L;
    for (int f = f_lo; f < f_hi; f += 2) {
      const bool hasB = f + 1 < f_hi;                         // wave-uniform
      const bool own = fr == 0 || hasB;
      float xc[16];
      {
        float (&xa)[8] = reinterpret_cast<float (&)[8]>(xc[0]);
        float (&xb)[8] = reinterpret_cast<float (&)[8]>(xc[8]);
        load_frame<4, 256>(arow, a.T, a.hop, f, lane, xa);
        load_frame<4, 256>(arow, a.T, a.hop, hasB ? f + 1 : f, lane, xb);
      }
      const float* trow = a.target + ((size_t)b * a.F + f + (own ? fr : 0)) * NB;
      float tk_[4], tq_[4], th_ = 0.0f;
#pragma unroll
      for (int e = 0; e < 4; ++e) { tk_[e] = trow[kl + 32 * e]; tq_[e] = trow[N2 - kl - 32 * e]; }
      if (kl == 0) th_ = trow[HALF];
      // ---- forward
      cpx u[8];
      {
        cpx v[8];
#pragma unroll
        for (int n1 = 0; n1 < 4; ++n1) {
          v[n1] = cmk(xc[2 * n1], xc[2 * n1 + 1]) * t_win[64 * n1];
          v[4 + n1] = cmk(xc[8 + 2 * n1], xc[8 + 2 * n1 + 1]) * t_win[64 * n1];
        }
        fft2(v, u);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) sA[fr * HALF + kl + 32 * e] = u[4 + e];
      wave_lds_sync();
      // ---- per bin pair (k, N2 - k): X, value, cotangent, the pair's two inverse inputs
      cpx zk_in[4], zn_in[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = kl + 32 * e;
        cpx zn = sA[fr * HALF + ((HALF - k) & (HALF - 1))];
        const cpx zk = u[e];
        if (e == 0 && k == 0) zn = zk;
        const cpx w = t_twu[64 * e];                              // W_N^k = e^{-2 pi i k / N}
        cpx xk, xq;
        bin_pair_unpack(zk, zn, w, xk, xq);
        const float vk = bl.value(xk.x * xk.x + xk.y * xk.y), vq = bl.value(xq.x * xq.x + xq.y * xq.y);
        const float gk = bl.value_grad(vk, tk_[e]), gq = bl.value_grad(vq, tq_[e]);
        const cpx ck = xk * (2.0f * bl.power_grad(gk, vk));          // G[k]
        const cpx cq = xq * (2.0f * bl.power_grad(gq, vq));          // G[N2 - k]
        if (e == 0 && k == 0) { zk_in[e] = cmk(ck.x + cq.x, ck.x - cq.x); zn_in[e] = zk_in[e]; }   // edge bins (real X): a[0] + i b[0]
      else bin_pair_adjoint(ck, cq, w, zk_in[e], zn_in[e]);
      }
      // bin HALF pairs with itself: X[HALF] = conj(Z[HALF]) (the lanes with kl = 0 hold Z[HALF] = u[4])
      cpx zh_in;
      {
        const cpx xh = cmk(u[4].x, -u[4].y);
        const float vh = bl.value(xh.x * xh.x + xh.y * xh.y);
        const float gh = bl.value_grad(vh, th_);
        const cpx ch = xh * (2.0f * bl.power_grad(gh, vh));
        zh_in = cmk(ch.x, -ch.y);
      }
      wave_lds_sync();                                            // every Z read is done
      // ---- conj(Zin) of both frames in natural order (frame-major, padded), then the lane's points of it
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = kl + 32 * e;
        sA[pad(fr * N2 + k)] = cmk(zk_in[e].x, -zk_in[e].y);
        if (k != 0) sA[pad(fr * N2 + N2 - k)] = cmk(zn_in[e].x, -zn_in[e].y);
      }
      if (kl == 0) sA[pad(fr * N2 + HALF)] = cmk(zh_in.x, -zh_in.y);
      wave_lds_sync();
      cpx r[8];
      {
        cpx v[8];
#pragma unroll
        for (int n1 = 0; n1 < 4; ++n1) { v[n1] = sA[pad(64 * n1 + lane)]; v[4 + n1] = sA[pad(N2 + 64 * n1 + lane)]; }
        wave_lds_sync();
        fft2(v, r);
      }
      wave_lds_sync();
      // ---- z[m] = conj(out[m]) = y[2m] + i y[2m+1], m = kl + 32 e: window, into the ring -- frame A's lanes, then B's
      // (the ring holds ONE frame length: frame A's first hop samples have to leave before frame B's last hop samples,
      // which wrap onto them, arrive -- per frame: add, then flush the hop samples no later frame reaches)
      const int rbA = ((f - f_lo) * a.hop) & (NFFT - 1);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (half == 1 && !hasB) break;                            // wave-uniform
        const int rb = (rbA + half * a.hop) & (NFFT - 1);
        if (fr == half) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int m = kl + 32 * e;
            const cpx w2 = t_wo[64 * e];
            cpx* rp = reinterpret_cast<cpx*>(ring + ((rb + 2 * m) & (NFFT - 1)));
            const cpx cur = *rp;
            *rp = cmk(cur.x + w2.x * r[e].x, cur.y - w2.y * r[e].y);
          }
        }
        wave_lds_sync();
        float* sp = span + (size_t)(f + half - f_lo) * a.hop;
        for (int i = lane; i < a.hop; i += 64) {
          const int idx = (rb + i) & (NFFT - 1);
          sp[i] = ring[idx];
          ring[idx] = 0.0f;
        }
        wave_lds_sync();
      }
    }
    if (f_hi > f_lo) {                                            // the chunk's tail: what is left in the ring
      const int nf = f_hi - f_lo, rb = (nf * a.hop) & (NFFT - 1);
      float* sp = span + (size_t)nf * a.hop;
      for (int i = lane; i < NFFT - a.hop; i += 64) {
        const int idx = (rb + i) & (NFFT - 1);
        sp[i] = ring[idx];
        ring[idx] = 0.0f;
      }
      wave_lds_sync();
    }
  }
}

// ---------------------------------------------------------------------------------------------------- host dispatch
static bool stft_v1() {   // diagnostics: the round-2 kernels
  static const int v1 = ias_diag_env("IAS_STFT_V1") ? atoi(ias_diag_env("IAS_STFT_V1")) : 0;
  return v1 != 0;
}

// chunks for `nwaves` resident waves: every wave one chunk of G consecutive frames (G hop >= n_fft - hop: a sample then
// lies in at most two chunk spans), chunks never cross rows.  Fills a.G / cper / L / nchunks and plan[3].
static bool span_plan(SgwArgs& a, int* plan, int B, int n_fft, long long nwaves) {
  const int F = a.F, hop = a.hop;
  long long cper0 = nwaves / B;
  if (cper0 < 1) cper0 = 1;
  int G = (int)((F + cper0 - 1) / cper0);
  const int gmin = (n_fft - hop + hop - 1) / hop;
  if (G < gmin) G = gmin;
  if (G >= F) G = F;
  const int cper = (F + G - 1) / G;
  const long long L = (long long)(G - 1) * hop + n_fft;
  if ((long long)B * cper * L > (long long)B * F * n_fft || (long long)B * cper > 2000000000LL) return false;
  a.G = G; a.cper = cper; a.L = (int)L; a.nchunks = B * cper;
  plan[0] = G; plan[1] = cper; plan[2] = (int)L;
  return true;
}

// what a stft_grad_wave_kernel launch needs beside the kernel's arguments
struct WaveLaunch {
  SgwArgs& a;
  int* plan;
  int B, n_fft, ncu;
  size_t lds, lds_static;
  dim3 grid;        // the frames form's; SPAN: from the chunk plan
  bool dry;
  hipStream_t stream;
};
template <int LOG2N, bool MEL, bool SPAN, bool CROW>
static int launch_wave(WaveLaunch w) {
  // (the shared-coefficient kernel answers for the chunk plan of both: ias_stft_grad_span_plan)
  if (w.lds + w.lds_static > 48 * 1024) {
    (void)hipFuncSetAttribute((const void*)stft_grad_wave_kernel<LOG2N, MEL, SPAN, false>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.lds);
    if (CROW)
      (void)hipFuncSetAttribute((const void*)stft_grad_wave_kernel<LOG2N, MEL, SPAN, CROW>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.lds);
  }
  if (SPAN) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, stft_grad_wave_kernel<LOG2N, MEL, SPAN, false>, 256, w.lds) != hipSuccess || nb < 1)
      nb = 1;
    if (!span_plan(w.a, w.plan, w.B, w.n_fft, (long long)w.ncu * nb * 4)) return IAS_ERR_UNSUPPORTED;
    if (w.dry) return IAS_OK;
    const long long need = ((long long)w.a.nchunks + 3) / 4;
    w.grid = dim3((unsigned)(need < (long long)w.ncu * nb ? need : (long long)w.ncu * nb));
  }
  hipLaunchKernelGGL((stft_grad_wave_kernel<LOG2N, MEL, SPAN, CROW>), w.grid, dim3(256), w.lds, w.stream, w.a);
  return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
}
template <bool MEL, bool SPAN, bool CROW>
static int launch_wave_nfft(const WaveLaunch& w) {
  if (w.n_fft == 512) {   // spans of linear bins are stft_grad512_kernel's: only IAS_STFT_V1 brings them here
    if constexpr (kIasDiag || MEL || !SPAN) return launch_wave<9, MEL, SPAN, CROW>(w);
    else return IAS_ERR_UNSUPPORTED;
  }
  if (w.n_fft == 1024) return launch_wave<10, MEL, SPAN, CROW>(w);
  return launch_wave<11, MEL, SPAN, CROW>(w);
}

// frame_grad [B,F,n_fft] <- d loss / d (windowed frames) (see stft_grad_wave_kernel); tables: ias_stft_build_tables of
// the plan's window; mel_*: the forward's CSR filterbank or NULL (linear bins, n_out = n_fft/2+1); target [B,F,n_out];
// coef: device doubles [2] (loss_mode 2, linear bins only).
// plan != NULL: the SPAN kernels (overlap-add inside the kernel); frame_grad then receives B * plan[1] chunk spans of
// plan[2] floats (plan[0] = frames per chunk), IAS_ERR_UNSUPPORTED when the shape does not allow it.
// CROW: coef is [B][2] (one pair per row, loss_mode 2, linear bins); the chunk plan is the one of the shared-coefficient
// kernels (their occupancy), so ias_stft_grad_span_plan answers for both.
template <bool CROW>
static int grad_frames_launch(const float* audio, const float* tables, const int* mel_start, const int* mel_count,
                              const int* mel_woff, const float* mel_w, int mel_nnz, int n_out, const float* target,
                              const double* coef, float* frame_grad, int B, int T, int n_fft, int hop, int power,
                              int loss_mode, float scale, float eps, int* plan, hipStream_t stream, bool dry = false) {
  if (!dry && (!audio || !tables || !target || !frame_grad)) return IAS_ERR_ARG;
  if (B <= 0 || B > 65535 || hop <= 0) return IAS_ERR_ARG;
  if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return IAS_ERR_UNSUPPORTED;
  if ((power != 1 && power != 2) || (loss_mode != 1 && loss_mode != 2) || (!dry && loss_mode == 2 && !coef)) return IAS_ERR_ARG;
  if (CROW && (loss_mode != 2 || power != 1 || mel_start != nullptr || mel_nnz > 0)) return IAS_ERR_ARG;
  const bool mel = mel_start != nullptr || (dry && mel_nnz > 0);
  if (!dry && mel && (!mel_count || !mel_woff || !mel_w || mel_nnz <= 0 || n_out <= 0 || loss_mode != 1)) return IAS_ERR_ARG;
  if (!mel && n_out != n_fft / 2 + 1) return IAS_ERR_ARG;
  const int F = ias_stft_num_frames(T, n_fft, hop);
  if (F < 0 || F > 2147483647 / n_fft) return IAS_ERR_ARG;
  const bool span = plan != nullptr;
  SgwArgs a;
  a.audio = audio; a.tables = tables; a.target = target; a.coef = coef; a.frame_grad = frame_grad;
  a.T = T; a.F = F; a.hop = hop; a.power2 = power == 2; a.loss_mode = loss_mode; a.scale = scale; a.eps = eps;
  a.mel_start = mel_start; a.mel_count = mel_count; a.mel_woff = mel_woff; a.mel_w = mel_w;
  a.n_out = n_out; a.mel_nnz = mel ? mel_nnz : 0;
  a.G = a.cper = a.L = a.nchunks = 0;
  static const int wgs_env = ias_diag_env("IAS_STFT_GRAD_WGS") ? atoi(ias_diag_env("IAS_STFT_GRAD_WGS")) : 0;   // diagnostics
  int per_row = (wgs_env > 0 ? wgs_env : 1024) / B;   // one resident round (measured: 2.36 -> 2.29 ms for the MR-STFT loss)
  if (per_row < 1) per_row = 1;
  int g = (F + per_row - 1) / per_row;
  if (g < 8) g = 8;
  a.groups = g;
  int ncu = 256, dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
  if (span && (hop > n_fft / 2 || (hop & 1) || (long long)B * F >= 2000000000LL)) return IAS_ERR_UNSUPPORTED;
  if (n_fft == 2048 && !mel && !stft_v1() && (long long)B * F < 2000000000LL && (reinterpret_cast<uintptr_t>(frame_grad) & 15) == 0 &&
      (!span || (hop & 3) == 0)) {
    constexpr int W2 = 8;
    const size_t lds2 = sizeof(cpx) * (W2 * 64 * IAS_S2_ROW + (span ? W2 * 1024 : 0));       // + 32 KB of static tables
    if (span) {
      if (!span_plan(a, plan, B, n_fft, (long long)ncu * W2)) return IAS_ERR_UNSUPPORTED;
      if (dry) return IAS_OK;
      const long long need = ((long long)a.nchunks + W2 - 1) / W2;
      const int grid2 = (int)(need < (long long)ncu ? need : (long long)ncu);
      (void)hipFuncSetAttribute((const void*)stft_grad2k_kernel<W2, true, CROW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
      hipLaunchKernelGGL((stft_grad2k_kernel<W2, true, CROW>), dim3(grid2), dim3(64 * W2), lds2, stream, a, B * F, 0u);
    } else {
      const long long need = ((long long)B * F + W2 - 1) / W2;
      const int grid2 = (int)(need < 2LL * ncu ? need : 2LL * ncu);
      (void)hipFuncSetAttribute((const void*)stft_grad2k_kernel<W2, false, CROW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
      hipLaunchKernelGGL((stft_grad2k_kernel<W2, false, CROW>), dim3(grid2), dim3(64 * W2), lds2, stream, a, B * F,
                         (F == 1 ? 0xFFFFFFFFu /* 2^32 / 1 does not fit: q0 = fi - 1, which row_of's one-step correction fixes */ : (unsigned)(0x100000000ULL / (unsigned long long)F)));
    }
    return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
  }
  if (n_fft == 512 && span && !mel && !stft_v1()) {
    constexpr int W5 = 8;
    const size_t lds5 = sizeof(cpx) * (W5 * 64 * IAS_S2_ROW) + sizeof(float) * W5 * 512;
    (void)hipFuncSetAttribute((const void*)stft_grad512_kernel<W5, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds5);
    if (CROW) (void)hipFuncSetAttribute((const void*)stft_grad512_kernel<W5, CROW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds5);
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, stft_grad512_kernel<W5, false>, 64 * W5, lds5) != hipSuccess || nb < 1) nb = 1;
    if (!span_plan(a, plan, B, n_fft, (long long)ncu * nb * W5)) return IAS_ERR_UNSUPPORTED;
    if (dry) return IAS_OK;
    const long long need = ((long long)a.nchunks + W5 - 1) / W5;
    const int grid5 = (int)(need < (long long)ncu * nb ? need : (long long)ncu * nb);
    hipLaunchKernelGGL((stft_grad512_kernel<W5, CROW>), dim3(grid5), dim3(64 * W5), lds5, stream, a);
    return hipGetLastError() == hipSuccess ? IAS_OK : IAS_ERR_LAUNCH;
  }
  const int R = n_fft / 128, scr = 8 * R * IAS_S2_ROW, np_it = (8 * R + 63) / 64, nunp = (n_fft / 4) / 64 + 1;
  const size_t lds_static = sizeof(float) * 64 * (2 * R + 2 * R + 16 * np_it + 2 * nunp);   // the kernel's table object
  size_t lds = sizeof(cpx) * 4 * scr + 16;
  if (span) lds += sizeof(float) * 4 * n_fft;
  if (mel)
    lds += sizeof(float) * (mel_padded_words(mel_nnz, n_out) + ((3 * n_out + 3) & ~3) +
                            4 * (((n_out + 3) & ~3) + n_fft / 2 + 1 + 7));
  if (lds + lds_static > 150 * 1024) return IAS_ERR_UNSUPPORTED;
  const WaveLaunch w = {a, plan, B, n_fft, ncu, lds, lds_static, dim3((F + g - 1) / g, B), dry, stream};
  if constexpr (!CROW) {   // CROW implies linear bins
    if (mel) return span ? launch_wave_nfft<true, true, false>(w) : launch_wave_nfft<true, false, false>(w);
  }
  return span ? launch_wave_nfft<false, true, CROW>(w) : launch_wave_nfft<false, false, CROW>(w);
}

extern "C" int ias_stft_grad_frames(const float* audio, const float* tables, const int* mel_start, const int* mel_count,
                                    const int* mel_woff, const float* mel_w, int mel_nnz, int n_out, const float* target,
                                    const double* coef, float* frame_grad, int B, int T, int n_fft, int hop, int power,
                                    int loss_mode, float scale, float eps, void* stream_) {
  return grad_frames_launch<false>(audio, tables, mel_start, mel_count, mel_woff, mel_w, mel_nnz, n_out, target, coef,
                                   frame_grad, B, T, n_fft, hop, power, loss_mode, scale, eps, nullptr, (hipStream_t)stream_);
}

// The chunk plan ias_stft_grad_spans will use for this shape (the device's occupancy enters it), without launching:
// plan_host[3] = {G, chunks per row, floats per chunk span}.  mel_nnz / n_out as for the launch (mel_nnz = 0: linear bins).
extern "C" int ias_stft_grad_span_plan(int B, int T, int n_fft, int hop, int mel_nnz, int n_out, int* plan_host) {
  if (!plan_host) return IAS_ERR_ARG;
  if (mel_nnz > 0 && (n_out <= 0 || n_out > n_fft / 2 + 1)) return IAS_ERR_ARG;
  return grad_frames_launch<false>(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, mel_nnz, n_out, nullptr, nullptr,
                                   nullptr, B, T, n_fft, hop, 1, 1, 1.0f, 0.0f, plan_host, nullptr, true);
}

// The same with the overlap-add inside the kernel: chunk_spans (B * plan[1] * plan[2] floats, 16-byte aligned) receives
// B * plan_host[1] spans of plan_host[2] floats, span c = row c / plan[1], frames [j G, j G + G) with j = c % plan[1],
// G = plan_host[0]: span[i] = sum over the chunk's frames f covering padded sample j G hop + i of window x frame
// gradient, in frame order.  stft_grad_combine_kernel (ias_stft_loss_backward) adds the (at most two) chunks per sample.
extern "C" int ias_stft_grad_spans(const float* audio, const float* tables, const int* mel_start, const int* mel_count,
                                   const int* mel_woff, const float* mel_w, int mel_nnz, int n_out, const float* target,
                                   const double* coef, float* chunk_spans, int B, int T, int n_fft, int hop, int power,
                                   int loss_mode, float scale, float eps, int* plan_host, void* stream_) {
  if (!plan_host || (reinterpret_cast<uintptr_t>(chunk_spans) & 15) != 0) return IAS_ERR_ARG;
  return grad_frames_launch<false>(audio, tables, mel_start, mel_count, mel_woff, mel_w, mel_nnz, n_out, target, coef,
                                   chunk_spans, B, T, n_fft, hop, power, loss_mode, scale, eps, plan_host,
                                   (hipStream_t)stream_);
}

// The per-row-coefficient forms of the two entries above for one resolution of the per-sound MR-STFT losses
// (MultiResolutionSTFTLoss.per_item): loss_mode 2, power 1, linear bins (n_out = n_fft / 2 + 1), coef_rows [B][2] device
// doubles (ias_mrstft_coef_rows), read at the row being processed.  A row whose pair is {0, 0} gets exactly 0.
extern "C" int ias_stft_grad_frames_mrstft_rows(const float* audio, const float* tables, int n_out, const float* target,
                                                const double* coef_rows, float* frame_grad, int B, int T, int n_fft,
                                                int hop, float eps, void* stream_) {
  if (!coef_rows) return IAS_ERR_ARG;
  return grad_frames_launch<true>(audio, tables, nullptr, nullptr, nullptr, nullptr, 0, n_out, target, coef_rows,
                                  frame_grad, B, T, n_fft, hop, 1, 2, 0.0f, eps, nullptr, (hipStream_t)stream_);
}

extern "C" int ias_stft_grad_spans_mrstft_rows(const float* audio, const float* tables, int n_out, const float* target,
                                               const double* coef_rows, float* chunk_spans, int B, int T, int n_fft,
                                               int hop, float eps, int* plan_host, void* stream_) {
  if (!coef_rows || !plan_host || (reinterpret_cast<uintptr_t>(chunk_spans) & 15) != 0) return IAS_ERR_ARG;
  return grad_frames_launch<true>(audio, tables, nullptr, nullptr, nullptr, nullptr, 0, n_out, target, coef_rows,
                                  chunk_spans, B, T, n_fft, hop, 1, 2, 0.0f, eps, plan_host, (hipStream_t)stream_);
}
