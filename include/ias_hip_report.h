/* Match report: loss-independent quality figures per sound (inverse-audio-synthesis_amd/report.py, match_audio.py
 * --report; csrc/report_kernels.hip).  Part of the product library (csrc/libias_hip.so) and of the diagnostic one; the
 * status codes and the conventions of include/ias_hip.h hold: device pointers unless said otherwise, contiguous fp32,
 * nothing allocated, freed or synchronised inside a call.  The reference never compares a match with its target by
 * anything but its own loss, so this has no counterpart there.
 *
 * ias_spectral_report: values V and target T [B, F, K] (fp32, frames-major: what ias_stft writes), floor_rows [B]
 *   (fp32, every entry > 0 and a normal number: NOT validated on the device), power 1 (magnitudes) or 2 (powers), dct
 *   NULL or a device copy of the ias_report_build_dct table [n_coef][K] -> out [B][5] device doubles
 *   {lsd_db, spectral_convergence, log_l1_db, mcd_db (0 without dct), n}.  Per row b with fl = floor_rows[b]:
 *     v' = max(v, fl), t' = max(t, fl), d = log2 v' - log2 t' (fp32, the hardware's __log2f as in the MR-STFT kernels:
 *       about 1 ulp on normal arguments, which the floor guarantees), a = (20 / power) log10 2 the dB of one log2 unit;
 *     frame f is COUNTED iff max_k max(v, t) > fl on the raw fp32 inputs, n = the number of counted frames; in an
 *       uncounted frame every d is exactly 0, so counting changes the divisors only (a note zero-padded to the buffer
 *       gets the figures of the note alone);
 *     lsd_db    = (a / n) sum_{counted f} sqrt((1/K) sum_k d^2);
 *     log_l1_db = (a / (n K)) sum_{counted f} sum_k |d|;
 *     spectral_convergence = sqrt(sum (t - v)^2) / sqrt(sum t^2) over ALL raw elements of the row; with a denominator
 *       of 0 it is 0 when the numerator is 0, else +inf;
 *     mcd_db    = (10 / ln 10) (1/n) sum_{counted f} sqrt(2 sum_{c=1..C} (sum_k D[c,k] (ln 2 / power) d[f,k])^2), C =
 *       n_coef, D the orthonormal DCT-II below without c = 0 (the overall level is lsd_db's business); by linearity the
 *       distance between the two sounds' cepstra of the clamped log values;
 *     n = 0: the three means are 0.
 *   Arithmetic: per frame the sums over k are fp32 chains per lane (lane l takes k = l, l + 64, ... in that order, fmaf
 *   for squares and products), folded across the 64 lanes in a fixed pattern of exchanges; the roots are taken per
 *   frame in fp32; frames are summed in fp64, in frame order within a wave's 8 consecutive frames, the 4 waves of a chunk of 32 frames
 *   in wave order, the chunks in chunk order; a, the divisors and the quotient are applied in fp64.
 *   Per-row contract (as ias_l1_rows and ias_envelope_frames): the assignment of frames to waves and chunks depends on
 *   F alone, so a row's five numbers are the same bits wherever the row sits in the batch, whatever B and whatever the
 *   4-byte alignment of the buffers.
 *   partials: scratch, [B][ias_spectral_report_partials_count(F)][6] doubles (per chunk of 32 frames: the two frame
 *   sums, the two convergence sums, the cepstral sum and the counted frames).
 *   IAS_ERR_ARG: a null values, target, floor_rows, partials or out; B, F or K < 1; power outside {1, 2}; with dct,
 *   n_coef < 1.  IAS_ERR_UNSUPPORTED: B > 65535; K > 2048; with dct, n_coef > 32, n_coef >= K or K > 256.  Nothing is
 *   launched on a refusal.  Without dct, n_coef is ignored.
 * ias_spectral_report_partials_count: chunks of 32 frames in F frames (records of 6 doubles per row); IAS_ERR_ARG when
 *   F < 1.
 * ias_report_build_dct (HOST only): out_host [n_coef][n_in] fp32, row c - 1 the coefficient c = 1 .. n_coef:
 *   D[c,k] = sqrt(2 / n_in) cos(pi c (2 k + 1) / (2 n_in)), torchaudio's create_dct(norm="ortho") without its row 0,
 *   computed in fp64 and rounded once.  IAS_ERR_ARG: a null pointer, n_in < 1 or n_coef < 1; IAS_ERR_UNSUPPORTED:
 *   n_coef >= n_in. */
#ifndef IAS_HIP_REPORT_H
#define IAS_HIP_REPORT_H
#include "ias_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int ias_report_build_dct(int n_in, int n_coef, float* out_host);
long long ias_spectral_report_partials_count(int F);
int ias_spectral_report(const float* values, const float* target, const float* floor_rows, const float* dct, int B, int F,
                        int K, int n_coef, int power, double* partials, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
