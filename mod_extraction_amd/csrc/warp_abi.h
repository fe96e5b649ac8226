/* warp_abi.h -- the C ABI of K26 (csrc/warp.hip): rows of fp32 audio read along a straight line of fractional positions,
 * for recorded dry / wet pairs whose two files were clocked by two crystals.  No counterpart in the reference.
 *
 * The conventions are those of include/modex_hip.h (status codes, pointer and scalar kinds, `stream`); the declarations live
 * here, and not there, until they are folded into that header together with an ABI number.  warp.hip includes this file,
 * so every definition is compiled against its declaration; mod_extraction_amd/_hip.py derives a fifth ctypes table
 * (SIGNATURES_WARP) from this text.  common.h does not include it.
 *
 * The function.  The prototype is K24's (resample_abi.h) at equal rates, all of it in fp64:
 *   c = rolloff,  half = ceil(zeros / c),  T = 2 half + 1;
 *   h(tau) = c sinc(c tau) I0(beta sqrt(1 - (tau / half)^2)) / I0(beta) for |tau| <= half, 0 beyond;
 *   sinc(x) = sin(pi x) / (pi x), sinc(0) = 1;  I0 by its power series sum_j ((beta'/2)^2)^j / (j!)^2, summed in ascending j
 *   until a term falls below 2^-60 of the sum.
 * Row b has offset[b] and drift[b] (fp64) and a sign s_b (+1, or -1 where sign[b] < 0; +1 without a sign array).
 * Output m of a row x of n_in samples (x is 0 outside 0 .. n_in - 1):
 *   pos = (double)m + ((double)m * drift + offset), each of the three operations rounded on its own (no fused multiply-add);
 *   i0 = floor(pos), f = pos - i0 (exact);  tau_k = f + (double)(half - k), one rounding;
 *   y[m] = fl32(s_b sum_{k = 0 .. T - 1} h(tau_k) x[i0 - half + k]): the taps are fp64 values and are not rounded to fp32; the
 *   sum is in fp64 in ascending k, one rounding at the end.  Terms whose x lies outside the row are left out, so an output
 *   whose window misses the row is s_b 0.
 * A tap the kernel evaluates may differ from h(tau_k) by at most 2^-40 in absolute value (the allowance K24's test grants a
 * tap of its table): sin(pi c (f + j)) comes by angle addition from one sincos per output and a table of T angles, except
 * for |tau| < 1, where it is evaluated directly; the series multiplies by a table of 1 / j^2 and the taps by 1 / I0(beta).
 * n_out is the caller's and independent of n_in.  With drift = 0 and an integer offset the taps are h(half - k): a
 * band-limited copy of x[m + offset], NOT a bit-exact one (the filter cuts above rolloff times Nyquist); a caller that
 * wants the samples themselves shifts by mx_pair_shift.
 * A row whose drift is not within +-MX_WARP_MAX_DRIFT or whose offset is not within +-MX_WARP_MAX_OFFSET (NaN included) --
 * they are device words the host cannot see without a synchronisation -- is written as n_out quiet NaNs. */
#ifndef MODEX_WARP_ABI_H
#define MODEX_WARP_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Limits: beyond them MX_ERR_UNSUPPORTED. */
#define MX_WARP_MAX_DRIFT 1e-3                      /* |drift| <= this: 1000 ppm, far beyond any crystal; rolloff needs
                                                       no scaling while rolloff (1 + this) <= 1, as the default 0.95 */
#define MX_WARP_MAX_OFFSET 2147483648.0             /* |offset| < this (2^31) */
#define MX_WARP_MAX_TAPS 4095                       /* T <= this, K24's cap */
#define MX_WARP_MAX_BETA 64.0                       /* beta <= this, K24's cap */
#define MX_WARP_MAX_N (1LL << 40)                   /* n_in, n_out <= this: m and pos stay exact integers in fp64 */
#define MX_WARP_OUT_TILE 1024                       /* outputs of one row a workgroup computes */
#define MX_WARP_MAX_ROWS 65535                      /* rows of one launch; more rows are more launches */

/* The plan of a warp: host arithmetic only, no device work; the four outputs are HOST words.  drift_bound and offset_bound
 * are what the caller knows of max |drift[b]| and max |offset[b]| (0 when it knows nothing: then only the kernel's per-row
 * test applies).
 * Checks, in this order.  MX_ERR_ARG: a NULL output; zeros < 1; rolloff not in (0, 1]; beta not >= 0 (NaN included); n_in
 * < 1 or n_out < 1; drift_bound or offset_bound not >= 0.  MX_ERR_UNSUPPORTED: beta > MX_WARP_MAX_BETA; T >
 * MX_WARP_MAX_TAPS; n_in or n_out > MX_WARP_MAX_N; more than 2^31 - 1 output tiles; drift_bound > MX_WARP_MAX_DRIFT;
 * offset_bound >= MX_WARP_MAX_OFFSET.  A refused plan writes nothing.
 * tiles = ceil(n_out / MX_WARP_OUT_TILE);  span = ceil(MX_WARP_OUT_TILE (1 + MX_WARP_MAX_DRIFT)) + T + 2: the input samples a
 * workgroup stages (it stages that many whatever the row's drift). */
int mx_warp_plan(int32_t zeros, double rolloff, double beta, int64_t n_in, int64_t n_out, double drift_bound,
                 double offset_bound, int32_t *half, int32_t *taps, int64_t *tiles, int32_t *span);

/* The warp: B rows of n_in floats x_stride apart -> B rows of n_out floats y_stride apart, rows starting at any 4-byte
 * boundary; offset and drift are device arrays of B doubles, sign a device array of B floats or NULL.
 * Grid (output tile, row), at most MX_WARP_MAX_ROWS rows a launch.  No atomics, no workspace; every y[m] of every row is
 * overwritten, nothing else is; the same arguments give the same bits.
 * Checks, in this order.  MX_ERR_ARG: NULL x, offset, drift or y; B, n_in or n_out < 1; x_stride < n_in; y_stride < n_out;
 * zeros < 1; rolloff not in (0, 1]; beta not >= 0.  MX_ERR_UNSUPPORTED: beta, T, n_in, n_out or the number of tiles beyond
 * the limits.  MX_ERR_ARG: y shares a byte with x, offset, drift or sign.  All before any launch. */
int mx_warp_rows(const float *x, int64_t x_stride, int64_t B, int64_t n_in, const double *offset, const double *drift,
                 const float *sign, int32_t zeros, double rolloff, double beta, float *y, int64_t y_stride, int64_t n_out,
                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_WARP_ABI_H */
