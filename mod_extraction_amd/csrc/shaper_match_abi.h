/* shaper_match_abi.h -- the C ABI of K27 (csrc/shaper_match.hip): one memoryless polynomial curve per clip that carries a
 * rendered wet (y_hat) onto a recorded one (y) that went through a saturating stage, forward and backward.  No counterpart
 * in the reference.
 *
 * The conventions are those of include/modex_hip.h (status codes, pointer and scalar kinds, `stream`); the declarations live
 * here, and not there, until they are folded into that header together with an ABI number.  shaper_match.hip includes this
 * file, so every definition is compiled against its declaration; mod_extraction_amd/_hip.py derives a sixth ctypes table
 * (SIGNATURES_SHAPER) from this text.  common.h does not include it.
 *
 * The function, for one row: x = y_hat, y = the recorded wet, both of N samples; all arithmetic in fp64 unless said.
 *   order P in 1 .. 7;  the powers p_1 < .. < p_K are the odd integers <= P, with `even` all integers 1 .. P (K <= 7).
 *   There is no constant term.
 *   S2 = sum x^2;  r = fl32(sqrt(S2 / N)), widened again;  t[n] = x[n] / r.
 *   M_m = sum_n t[n]^m for every m = p_i + p_j (the even m in 2 .. 2 p_K, with `even` every m in 2 .. 2 P), the powers of t
 *   formed by repeated multiplication by t;  b_k = sum_n t[n]^(p_k) (y[n] / r);  E = sum y^2.
 *   A[i][j] = M_(p_i + p_j), its diagonal multiplied by (1 + ridge).  There is no absolute eps: the fit is exactly
 *   independent of r, and the backward treats r as a constant.  c = A^-1 b by Cholesky, rounded once to fp32.
 *   z[n] = fl32(r C(t[n])),  C(t) = sum_k c_k t^(p_k) by Horner from the fp32 c and r: with `even`
 *   t (c_1 + t (c_2 + ..)), else t (c_1 + s (c_3 + s (c_5 + s c_7))) with s = t t; every operation rounded on its own.
 *   flags: 1 = S2 or r is not positive or not finite, or a Cholesky pivot is not positive or not finite;
 *          2 = not (sum_k |fl32(c_k)| <= max_gain).
 *   A flagged row gets the identity (c_1 = 1, the rest 0; z = x bit for bit) and passes its gradient through unchanged; its
 *   scale is r, or 1 where r itself was refused.
 *   backward, dz given:  g_k = sum_n dz[n] t[n]^(p_k),  u = A^-1 g,  U(t) = sum_k u_k t^(p_k),
 *   dy_hat[n] = dz[n] C'(t) + U'(t) y[n] / r - (U'(t) C(t) + U(t) C'(t)) - 2 ridge sum_k u_k c_k p_k t^(2 p_k - 1),
 *   rounded once to fp32.  y gets no gradient.  The update is elementwise: dy_hat may be dz.
 *
 * Layout of the sums (n_sums = 1 + n_m + K + 1 doubles):  S2;  the n_m moments in ascending m;  b_1 .. b_K;  E.
 * The partials workspace is (B, n_chunks, n_sums) doubles, n_chunks = ceil(N / MX_SHAPER_CHUNK), and needs no initial
 * value; the backward's is (B, n_chunks, K).  Rows are a row stride apart and may start at any 4-byte boundary.  No atomics;
 * every reduction has a fixed order (lanes by butterfly, the four waves through LDS, the chunks lane by lane in ascending
 * order), so the same arguments give the same bits.
 *
 * Checks of every entry point, in this order, all before any launch.  MX_ERR_ARG: a NULL pointer, B or N < 1, a stride
 * below N, n_chunks != ceil(N / MX_SHAPER_CHUNK) where it is passed; order outside 1 .. MX_SHAPER_MAX_ORDER, even not 0 or
 * 1; ridge not a finite number >= 0, max_gain not a finite number >= 1.  MX_ERR_UNSUPPORTED: N > MX_SHAPER_MAX_N or B >
 * MX_SHAPER_MAX_ROWS.  MX_ERR_ARG: an output shares a byte with an input (dy_hat may be dz itself, with dz's stride). */
#ifndef MODEX_SHAPER_MATCH_ABI_H
#define MODEX_SHAPER_MATCH_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_SHAPER_CHUNK 2048                        /* samples of one row a workgroup owns */
#define MX_SHAPER_MAX_ORDER 7
#define MX_SHAPER_MAX_N 16777216                    /* 2^24 samples a row */
#define MX_SHAPER_MAX_ROWS 65535                    /* rows of one launch */

/* Two launches: the chunks' sums of x^2 (slot 0 of every chunk), then -- every workgroup re-reducing its row's S2 to the
 * same r -- the chunks' moments, cross sums and E (the other slots). */
int mx_shaper_match_partials(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B, int64_t N,
                             int32_t order, int32_t even, double *partials, void *stream);

/* One wave a row: the row's sums from its chunks, r, the Cholesky, the guards.  coeffs (B, K) fp32, scale (B,) fp32,
 * sums (B, n_sums) fp64, flags (B,) int32. */
int mx_shaper_match_solve(const double *partials, int64_t B, int64_t N, int64_t n_chunks, int32_t order, int32_t even,
                          double ridge, double max_gain, float *coeffs, float *scale, double *sums, int32_t *flags,
                          void *stream);

/* z = fl32(r C(y_hat / r)), elementwise; a flagged row is copied. */
int mx_shaper_match_apply(const float *y_hat, int64_t y_hat_stride, const float *coeffs, const float *scale,
                          const int32_t *flags, int64_t B, int64_t N, int32_t order, int32_t even, float *z, int64_t z_stride,
                          void *stream);

/* The chunks' g_k = sum dz t^(p_k) into partials (B, n_chunks, K); scale is the forward's. */
int mx_shaper_match_bwd_partials(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride,
                                 const float *scale, int64_t B, int64_t N, int32_t order, int32_t even, double *partials,
                                 void *stream);

/* One wave a row: g from its chunks, A from the forward's sums, u = A^-1 g (B, K) fp64; u = 0 on a flagged row. */
int mx_shaper_match_bwd_solve(const double *partials, const double *sums, const int32_t *flags, int64_t B, int64_t n_chunks,
                              int32_t order, int32_t even, double ridge, double *u, void *stream);

/* dy_hat, elementwise; a flagged row copies dz.  dy_hat may be dz (the same pointer and stride). */
int mx_shaper_match_bwd_apply(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride, const float *y,
                              int64_t y_stride, const float *coeffs, const float *scale, const double *u, const int32_t *flags,
                              int64_t B, int64_t N, int32_t order, int32_t even, double ridge, float *dy_hat,
                              int64_t dy_hat_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_SHAPER_MATCH_ABI_H */
