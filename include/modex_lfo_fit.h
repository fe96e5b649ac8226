/* modex_lfo_fit.h -- the part of the C ABI of libmodex_hip.so that round 18 added: the LFO fit (K18), the inverse of
 * mx_lfo_synth.  modex_hip.h includes this file at its end, beside modex_fx_head.h and for the same reason: the text of
 * modex_hip.h and _hip.SIGNATURES are held to each other and to a fixed count by the suite, so added entry points have a
 * header of their own and a binding table of their own (mod_extraction_amd/_hip.py: FIT_SIGNATURES).  mx_abi_version() is
 * that of modex_hip.h: entry points are only added. */
#ifndef MODEX_LFO_FIT_H
#define MODEX_LFO_FIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- K18: rate, phase and shape of LFO rows (csrc/lfo_fit.hip) -- no counterpart in the reference.
 * y: B rows of n fp32 points, y_stride floats apart; sr: the rate of the points in Hz; [f_min, f_max]: the rate window in Hz;
 * shape_mask: bit s allows shape id s (0 cos, 1 rect_cos, 2 inv_rect_cos, 3 tri, 4 saw, 5 rsaw, 6 sqr).
 *
 * A candidate (shape s, rate f, centre phase phic) has the template t_i = the value mx_lfo_synth writes at point i for
 * (fl32(f), ph, s, exp = 1, start = 0), where ph makes the template's own argument at position (n + 1) / 2 equal phic:
 *   ph_eff = (phic - step_eff (n + 1) / 2) mod 2 pi (step_eff: the fp32 phase step of the shape, the halved one for the
 *   rectified cosines);  ph = ph_eff, or 2 (ph_eff mod pi) for the rectified cosines;  fp64, rounded to fp32 once; a value
 *   that rounds to fl32(2 pi) becomes 0, so 0 <= ph < 2 pi.
 * Objective, fp64 in a fixed order, yc = y - mean(y), tc = t - mean(t):  Syy = sum yc^2, Stt = sum tc^2, Sty = sum tc yc,
 *   a = Sty / Stt if Stt > 0 and Sty > 0, else 0 (a >= 0: with a free sign saw / rsaw and rect_cos / inv_rect_cos are one
 *   family);  R = Syy - a Sty;  b = mean(y) - a mean(t).
 * Search per allowed shape: the grid f_k = f_min + k df, df = sr / (rate_div n), k < K = floor((f_max - f_min) / df) + 1,
 * phi_j = j (2 pi / J), j < J: argmin R, ties to the lowest (k, j); then rounds l = 1..L over the 5 x 5 points
 * f0 + i df / 2^l (clamped into the window), (phi0 + j (2 pi / J) / 2^l) mod 2 pi, i, j = -2..2, visited in (i, j) order, a
 * point replacing the best only where R is strictly smaller.  Then the argmin over the shapes, ties to the lowest id.
 *
 * Outputs (B,), each one fp32 rounding of the fp64 quantity: shape (int32), rate_hz = fl32(f), phase = ph, amp = a,
 * offset = b, resid = R / Syy; per_shape_resid (B, 7) is optional and holds each shape's R / Syy, +inf where not allowed.
 * offset + amp * mx_lfo_synth(rate_hz, phase, shape) is the best template bit for bit.  A constant row (Syy == 0) returns the
 * lowest allowed shape, rate f_min, phase 0, amp 0, offset its mean, resid 0; a row no candidate correlates positively with
 * returns amp 0, resid 1.  One launch, one workgroup per row, no atomics, no workspace: deterministic.
 * NULL required pointer, B <= 0, f_min <= 0, f_max < f_min, f_max >= sr / 2, an empty mask or bits above 6, L < 0,
 * y_stride < n: MX_ERR_ARG; n outside [16, 4096], K > 512, J outside [4, 128], L > 8, rate_div outside [1, 16]:
 * MX_ERR_UNSUPPORTED; all before any launch.  K == 1 (f_min == f_max) fits phase and shape at a known rate. */
int mx_lfo_fit(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, float f_min, float f_max, int32_t shape_mask,
               int32_t rate_div, int32_t J, int32_t L, int32_t *shape, float *rate_hz, float *phase, float *amp, float *offset,
               float *resid, float *per_shape_resid, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_LFO_FIT_H */
