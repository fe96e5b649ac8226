/*
 * modex_hip_fir.h -- the second header of the C ABI of libmodex_hip.so: the six entry points of K21.
 *
 * It exists only because the declaration count of modex_hip.h (117) and the ABI number (21) are pinned by tests that the
 * change which added K21 could not touch.  Folding these six declarations back into modex_hip.h (118..123, one header
 * again) is the follow-up.  Until then the same rules hold here as there: every entry point is `int mx_name(params);`, a
 * parameter is a pointer or one of int64_t, int32_t, uint64_t, uint32_t, float, double; csrc/common.h includes this file
 * too, so every definition is compiled against its declaration; mod_extraction_amd/_hip.py derives SIGNATURES_FIR from
 * this text.  Pointers, streams and return values: the conventions at the top of modex_hip.h (MX_OK, MX_ERR_*).
 */
#ifndef MODEX_HIP_FIR_H
#define MODEX_HIP_FIR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- K21: one short least-squares FIR per clip (csrc/fir_match.hip) -- no counterpart in the reference.
 * x = y_hat (the rendered wet), y (the recorded wet): B rows of N fp32 samples, a row stride (in floats, >= N) apart, both
 * zero outside [0, N).  K taps, 1 <= K <= MX_FIR_MAX_TAPS; a centre c, 0 <= c < K.  The matched signal is
 *
 *   z[n] = sum_{k < K} h[k] x[n + c - k],   n = 0 .. N - 1
 *
 * and the taps are the autocorrelation-method least-squares solution, fitted on the zero-extended signals:
 *
 *   R[d] = sum_n x[n] x[n + d]        (d = 0 .. K - 1)
 *   b[j] = sum_n x[n + c - j] y[n]    (j = 0 .. K - 1)
 *   E    = sum_n y[n]^2
 *   A    = toeplitz(R) + lambda I,    lambda = eps + ridge R[0]
 *   h    = A^-1 b                     (Cholesky A = L L^T in fp64, two triangular solves)
 *
 * Every sum is a sum of exact products of fp32 values accumulated in fp64 in one fixed order, |sum - exact| <=
 * N 2^-53 sum |terms|.  h is rounded once to fp32 and applied as fp32 values; z is accumulated in fp64 in the order
 * k = 0 .. K - 1 and rounded once.  A tap that is exactly 0 reads nothing (so the identity filter copies its row).
 * Two guards, each a bit of the row's flag:
 *   1  a pivot of the Cholesky that is not positive or not finite (h is not formed)
 *   2  not (sum |h| <= max_gain), h before the rounding (a NaN tap trips it too)
 * A flagged row uses the identity filter, h[c] = 1 and the rest 0, and its gradient passes through unchanged.  There is
 * no branch for a silent y_hat: eps > 0 gives h = 0.  K = 1 is K20's "ls" gain with eps' = eps + ridge R[0].
 *
 * Backward, with dz = d loss / d z (zero outside [0, N)) and the fp32 h the forward applied:
 *
 *   gh[k] = sum_n dz[n] x[n + c - k]
 *   u     = A^-1 gh
 *   s[d]  = sum_{k - j = d} (h[k] u[j] + u[k] h[j]),   d = -(K - 1) .. K - 1      (2K - 1 taps, s[-d] = s[d])
 *   s[0] += 2 ridge <u, h>                             (lambda depends on x through R[0])
 *   dy_hat[i] = sum_k h[k] dz[i + k - c] + sum_k u[k] y[i + k - c] - sum_d s[d] x[i + d]
 *
 * accumulated in fp64 in that order (k up, k up, d up) and rounded once; u = 0 and s = 0 on a flagged row, and zero
 * coefficients read nothing.  y gets no gradient.  dy_hat may not be dz: a sample's gradient reads its neighbours' dz.
 *
 * A workgroup owns MX_FIR_CHUNK samples of one row: n_chunks = ceil(N / MX_FIR_CHUNK); the `partials` and `apply`
 * launches have grid (n_chunks, B), the two `solve` launches one workgroup per row, which adds the chunks' partials in
 * the order 0, 1, 2, ...  No atomics: the same arguments give the same bits.  Rows are read in place wherever they start.
 * All six, before any launch: a NULL pointer, B < 1, N < 1, a stride < N, c outside [0, K) (for 1 <= K <= 32), ridge that
 * is not a finite number >= 0, eps that is not a finite number above 0, max_gain that is not a finite number >= 1, an
 * output that overlaps an input: MX_ERR_ARG.  K < 1, K > 32, N > 2^24, B > 65535: MX_ERR_UNSUPPORTED. */
#define MX_FIR_CHUNK 2048
#define MX_FIR_MAX_TAPS 32

/* partials: (B, n_chunks, 2K + 1) fp64 = the chunk's share of R[0 .. K-1], b[0 .. K-1], E. */
int mx_fir_match_partials(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B, int64_t N,
                          int64_t K, int64_t centre, double *partials, void *stream);

/* partials: what mx_fir_match_partials wrote.  taps (B, K) fp32 = the applied h; sums (B, 2K + 1) fp64 = R, b, E of the
 * row; flags (B,) int32. */
int mx_fir_match_solve(const double *partials, int64_t B, int64_t n_chunks, int64_t K, int64_t centre, double ridge,
                       double eps, double max_gain, float *taps, double *sums, int32_t *flags, void *stream);

/* z[b, n] = sum_k taps[b, k] x[b, n + c - k]: any (B, K) taps.  z: B rows z_stride apart; it may not overlap x or taps. */
int mx_fir_match_apply(const float *x, int64_t x_stride, const float *taps, int64_t B, int64_t N, int64_t K, int64_t centre,
                       float *z, int64_t z_stride, void *stream);

/* partials: (B, n_chunks, K) fp64 = the chunk's share of gh[0 .. K-1]. */
int mx_fir_match_bwd_partials(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride, int64_t B,
                              int64_t N, int64_t K, int64_t centre, double *partials, void *stream);

/* partials: what mx_fir_match_bwd_partials wrote; sums, taps, flags: what mx_fir_match_solve wrote (A is built again from
 * R = sums[:, :K] with the forward's ridge and eps).  u (B, K) and s (B, 2K - 1; s[b, K - 1 + d] for lag d) fp64. */
int mx_fir_match_bwd_solve(const double *partials, const double *sums, const float *taps, const int32_t *flags, int64_t B,
                           int64_t n_chunks, int64_t K, double ridge, double eps, double *u, double *s, void *stream);

/* dy_hat: B rows dy_hat_stride apart; it may overlap none of dz, y, y_hat, taps, u, s. */
int mx_fir_match_bwd_apply(const float *dz, int64_t dz_stride, const float *y, int64_t y_stride, const float *y_hat,
                           int64_t y_hat_stride, const float *taps, const double *u, const double *s, int64_t B, int64_t N,
                           int64_t K, int64_t centre, float *dy_hat, int64_t dy_hat_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_HIP_FIR_H */
