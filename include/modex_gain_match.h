/* modex_gain_match.h -- the part of the C ABI of libmodex_hip.so that round 21 added: the per-clip gain match of a rendered
 * wet against a recorded one (K20).  modex_hip.h includes this file at its end, beside modex_fx_head.h, modex_lfo_fit.h and
 * modex_pair_align.h and for the same reason: the text of modex_hip.h and _hip.SIGNATURES are held to each other and to a
 * fixed count by the suite, so added entry points have a header of their own and a binding table of their own
 * (mod_extraction_amd/_hip.py: GAIN_SIGNATURES).  mx_abi_version() is that of modex_hip.h: entry points are only added. */
#ifndef MODEX_GAIN_MATCH_H
#define MODEX_GAIN_MATCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- K20: one gain per clip (csrc/gain_match.hip) -- no counterpart in the reference.
 * y_hat (the rendered wet), y (the recorded wet): B rows of N fp32 samples, a row stride (in floats, >= N) apart.
 *
 *   a = <y_hat, y_hat>,  c = <y_hat, y>,  e = <y, y>                      (fp64 sums of exact products, fixed order)
 *   mode MX_GAIN_LS:   g = c / (a + eps)                                   (least squares)
 *   mode MX_GAIN_RMS:  g = sqrt((e + eps) / (a + eps))                     (energy match)
 *   clamp != 0: g < lo -> lo, g > hi -> hi, and the row is flagged; 0 < lo <= 1 <= hi.  clamp == 0: lo and hi are not read.
 *   g is rounded once to fp32;  z = fl32(g * y_hat)                        (one fp32 multiplication)
 * There is no branch for a silent row: eps > 0 keeps every quotient finite (a silent y_hat: "ls" g = 0, then the clamp).
 *
 * Backward, with dz = d loss / d z, s = <dz, y_hat> and the fp32 g the forward applied:
 *   MX_GAIN_LS,  row not flagged:  dy_hat = g dz + s (y - 2 g y_hat) / (a + eps)
 *   MX_GAIN_RMS, row not flagged:  dy_hat = g dz - s g y_hat / (a + eps)
 *   a flagged row, either mode:    dy_hat = g dz
 * each element formed in fp64 and rounded once.  y gets no gradient.
 *
 * A workgroup owns MX_GAIN_CHUNK samples of one row: n_chunks = ceil(N / MX_GAIN_CHUNK), grid (n_chunks, B).  The two
 * `partials` launches write one fp64 partial sum per workgroup into a caller-supplied workspace; the two `apply` launches
 * re-reduce the n_chunks partials of their row in one fixed order in every workgroup.  No atomics: the same arguments give
 * the same bits.  |sum - exact| <= N 2^-53 sum |terms|.
 * All four, before any launch: a NULL pointer, B < 1, N < 1, a stride < N, a mode other than the two, eps that is not a
 * finite number above 0, clamp != 0 with a range outside 0 < lo <= 1 <= hi, an output that overlaps an input (but
 * dy_hat == dz with the same stride): MX_ERR_ARG.  N > 2^24, B > 65535: MX_ERR_UNSUPPORTED. */
#define MX_GAIN_CHUNK 2048
#define MX_GAIN_LS 0
#define MX_GAIN_RMS 1

/* partials: (B, n_chunks, 3) fp64 = the partial a, c, e of every chunk. */
int mx_gain_match_partials(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B, int64_t N,
                           double *partials, void *stream);

/* partials: what mx_gain_match_partials wrote for the same rows.  z: B rows z_stride apart; it may not overlap y_hat
 * (the backward reads the un-matched rows).  gain (B,) fp32, sums (B, 3) fp64 = a, c, e, flags (B,) int32 (1 = clamped):
 * written by the workgroup of chunk 0. */
int mx_gain_match_apply(const float *y_hat, int64_t y_hat_stride, const double *partials, int64_t B, int64_t N, int32_t mode,
                        double eps, int32_t clamp, double lo, double hi, float *z, int64_t z_stride, float *gain,
                        double *sums, int32_t *flags, void *stream);

/* partials: (B, n_chunks) fp64 = the partial s of every chunk. */
int mx_gain_match_bwd_partials(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride, int64_t B,
                               int64_t N, double *partials, void *stream);

/* gain, sums, flags: what mx_gain_match_apply wrote; partials: what mx_gain_match_bwd_partials wrote.  dy_hat may be dz
 * itself (same pointer, same stride: the in-place update); it may overlap nothing else that is read. */
int mx_gain_match_bwd_apply(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride, const float *y,
                            int64_t y_stride, const float *gain, const double *sums, const int32_t *flags,
                            const double *partials, int64_t B, int64_t N, int32_t mode, double eps, float *dy_hat,
                            int64_t dy_hat_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_GAIN_MATCH_H */
