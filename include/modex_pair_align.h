/* modex_pair_align.h -- the part of the C ABI of libmodex_hip.so that round 20 added: the lag and polarity estimate of
 * recorded dry / wet pairs (K19).  modex_hip.h includes this file at its end, beside modex_fx_head.h and modex_lfo_fit.h and
 * for the same reason: the text of modex_hip.h and _hip.SIGNATURES are held to each other and to a fixed count by the suite,
 * so added entry points have a header of their own and a binding table of their own (mod_extraction_amd/_hip.py:
 * ALIGN_SIGNATURES).  mx_abi_version() is that of modex_hip.h: entry points are only added. */
#ifndef MODEX_PAIR_ALIGN_H
#define MODEX_PAIR_ALIGN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- K19: constant lag and polarity of dry / wet rows (csrc/pair_align.hip) -- no counterpart in the reference.
 * dry, wet: B rows of N fp32 samples, dry_stride / wet_stride floats apart; l runs over -L..L, 0 <= L < N.
 *
 *   r[b, l + L] = sum_n dry[b, n] wet[b, n + l]   over the n with both indices in [0, N)
 *   c           = r / sqrt(sum dry^2 sum wet^2)   (the energies of the whole rows)
 *   lag         = the l of the largest |c|; ties go to the smallest |l|, then to the non-negative one
 *   corr        = the signed c at lag; the polarity is its sign
 *   frac        = 0.5 (a - c+) / (a - 2 b0 + c+) with a, b0, c+ = |c| at lag - 1, lag, lag + 1: the vertex of the parabola
 *                 through the three; 0 at the window's two edges (lag = -L or L) or where the denominator is 0
 *   a row whose dry or wet energy is 0: lag 0, corr 0, frac 0
 * Convention: wet[n + lag] ~ sign(corr) dry[n]; a wet that is late by d samples has lag = +d.
 *
 * Every sum is fp64 in a fixed order (the product of two fp32 values is exact in fp64), no atomics, no workspace: the same
 * arguments give the same bits.  |r - exact| <= N 2^-53 sum |dry wet|.
 * All three: a NULL required pointer, B <= 0, N <= 0, a stride < N: MX_ERR_ARG; N > 2^24, B > 65535: MX_ERR_UNSUPPORTED;
 * xcorr and peak also L < 0 or L >= N: MX_ERR_ARG, L > 8192: MX_ERR_UNSUPPORTED; all before any launch. */

/* r_out: (B, 2 L + 1) fp64, contiguous.  Grid (tile of 64 lags, row); one lag a lane. */
int mx_pair_xcorr(const float *dry, int64_t dry_stride, const float *wet, int64_t wet_stride, int64_t B, int64_t N, int64_t L,
                  double *r_out, void *stream);

/* r: what mx_pair_xcorr wrote for the same rows.  Outputs (B,): lag_out int32, corr_out and frac_out fp32, each one rounding
 * of the fp64 quantity.  One workgroup a row. */
int mx_pair_peak(const float *dry, int64_t dry_stride, const float *wet, int64_t wet_stride, const double *r, int64_t B,
                 int64_t N, int64_t L, int32_t *lag_out, float *corr_out, float *frac_out, void *stream);

/* out[b, n] = s_b wet[b, n + lag[b]], 0 where n + lag[b] leaves [0, N); s_b = -1 where corr[b] < 0, else +1 (corr may be
 * NULL: s_b = +1).  lag: (B,) int32, any value; out rows out_stride floats apart.  With mx_pair_peak's lag and corr,
 * out ~ dry.  out may not overlap wet: MX_ERR_ARG. */
int mx_pair_shift(const float *wet, int64_t wet_stride, int64_t B, int64_t N, const int32_t *lag, const float *corr,
                  float *out, int64_t out_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_PAIR_ALIGN_H */
