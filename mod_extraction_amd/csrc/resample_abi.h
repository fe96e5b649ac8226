/* resample_abi.h -- the C ABI of K24 (csrc/resample.hip): band-limited rational sample-rate conversion of rows of fp32
 * audio, for recordings that were not made at the training rate.  No counterpart in the reference.
 *
 * The conventions are those of include/modex_hip.h (status codes, pointer and scalar kinds, `stream`); the declarations live
 * here, and not there, until they are folded into that header together with an ABI number.  resample.hip includes this file,
 * so every definition is compiled against its declaration; mod_extraction_amd/_hip.py derives a third ctypes table
 * (SIGNATURES_RESAMPLE) from this text.  common.h does not include it.
 *
 * The function.  From sr_in, sr_out (positive integers), zeros, rolloff and beta:
 *   g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g;
 *   c = rolloff * (up < down ? up / down : 1) in fp64: the cut-off as a fraction of the INPUT Nyquist frequency;
 *   half = ceil(zeros / c) in fp64, T = 2 half + 1 taps a phase;  n_out = ceil(n_in up / down) in 64-bit integers.
 * Prototype, tau in input samples, all of it in fp64:
 *   h(tau) = c sinc(c tau) I0(beta sqrt(1 - (tau / half)^2)) / I0(beta) for |tau| <= half, 0 beyond;
 *   sinc(x) = sin(pi x) / (pi x), sinc(0) = 1;  I0 by its power series sum_j ((beta'/2)^2)^j / (j!)^2, summed in ascending j
 *   until a term falls below 2^-60 of the sum.
 * Tap table, p in 0 .. up - 1, k in 0 .. T - 1, row-major (up, T):
 *   taps[p][k] = fl32(h(tau)), tau = ((half - k) up + p) / up  (the integer numerator is exact, one fp64 division).
 * Output m of a row x of n_in samples (x is 0 outside 0 .. n_in - 1):
 *   (i0, p) = divmod(m down, up) in 64-bit integers;
 *   y[m] = fl32(sum_{k = 0 .. T - 1} taps[p][k] x[i0 - half + k]): each product exact in fp64 (fp32 times fp32), summed in
 *   fp64 in ascending k, one rounding.  Terms whose x lies outside the row are left out (they are exact zeros).
 * This is scipy.signal.resample_poly(x, up, down, window=proto / up) with proto[j + half up] = h(j / up). */
#ifndef MODEX_RESAMPLE_ABI_H
#define MODEX_RESAMPLE_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Limits: beyond them MX_ERR_UNSUPPORTED. */
#define MX_RESAMPLE_MAX_FACTOR 4096                 /* up, down <= this */
#define MX_RESAMPLE_MAX_TAPS 4095                   /* T <= this */
#define MX_RESAMPLE_MAX_TABLE (1 << 24)             /* up T <= this many floats */
#define MX_RESAMPLE_MAX_SPAN (1LL << 62)            /* n_in up < this */
#define MX_RESAMPLE_MAX_BETA 64.0                   /* beta <= this (I0 stays far inside fp64) */
#define MX_RESAMPLE_OUT_TILE 4096                   /* outputs of one row a workgroup computes */
#ifndef MX_RESAMPLE_LDS_TABLE_BYTES
#define MX_RESAMPLE_LDS_TABLE_BYTES (160 * 1024)    /* a table of at most this many bytes is staged in LDS */
#endif
/* route */
#define MX_RESAMPLE_ROUTE_LDS 0                     /* every workgroup stages the whole table in LDS */
#define MX_RESAMPLE_ROUTE_L2 1                      /* the table does not fit: taps are read through L1 / L2 */

/* The plan of a conversion: host arithmetic only, no device work; the six outputs are HOST words.
 * Checks, in this order.  MX_ERR_ARG: a NULL output; sr_in < 1 or sr_out < 1; zeros < 1; rolloff not in (0, 1]; beta not
 * >= 0 (NaN included); n_in < 1.  MX_ERR_UNSUPPORTED: beta > MX_RESAMPLE_MAX_BETA; up or down > MX_RESAMPLE_MAX_FACTOR;
 * T > MX_RESAMPLE_MAX_TAPS; up T > MX_RESAMPLE_MAX_TABLE; n_in up >= MX_RESAMPLE_MAX_SPAN; more than 2^31 - 1 output tiles.
 * A refused plan writes nothing.  table_floats = up T;  route = MX_RESAMPLE_ROUTE_LDS when 4 up T <=
 * MX_RESAMPLE_LDS_TABLE_BYTES, else MX_RESAMPLE_ROUTE_L2. */
int mx_resample_plan(int64_t sr_in, int64_t sr_out, int32_t zeros, double rolloff, double beta, int64_t n_in, int32_t *up,
                     int32_t *down, int32_t *half, int64_t *n_out, int64_t *table_floats, int32_t *route);

/* The tap table: taps (up, T) fp32 on the device, any 4-byte boundary; one thread per entry, in fp64, one rounding.
 * Checks, in this order.  MX_ERR_ARG: NULL taps; up, down or half < 1; gcd(up, down) != 1; rolloff not in (0, 1]; beta not
 * >= 0.  MX_ERR_UNSUPPORTED: beta, up, down, T or up T beyond the limits.  Every entry is overwritten. */
int mx_resample_taps(int32_t up, int32_t down, int32_t half, double rolloff, double beta, float *taps, void *stream);

/* The conversion: B rows of n_in floats x_stride apart -> B rows of n_out floats y_stride apart, rows starting at any
 * 4-byte boundary; taps as mx_resample_taps wrote them (any (up, 2 half + 1) table is applied as it stands).
 * Grid (output tile, row), at most 65535 rows a launch; the route is the plan's.  No atomics, no workspace; every y[m] of
 * every row is overwritten, nothing else is; the same arguments give the same bits.
 * Checks, in this order.  MX_ERR_ARG: NULL x, taps or y; B, n_in or n_out < 1; x_stride < n_in; y_stride < n_out; up, down
 * or half < 1; gcd(up, down) != 1.  MX_ERR_UNSUPPORTED: up, down, T, up T, n_in up or the number of tiles beyond the limits.
 * MX_ERR_ARG: n_out != ceil(n_in up / down); y shares a byte with x or with the table.  All before any launch. */
int mx_resample_rows(const float *x, int64_t x_stride, int64_t B, int64_t n_in, int32_t up, int32_t down, int32_t half,
                     const float *taps, float *y, int64_t y_stride, int64_t n_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_RESAMPLE_ABI_H */
