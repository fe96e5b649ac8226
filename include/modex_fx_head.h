/* modex_fx_head.h -- the part of the C ABI of libmodex_hip.so that round 17 added: the per-clip effect-parameter head (K17).
 * modex_hip.h includes this file at its end, so a user of that header has these declarations too; they are kept in a file
 * of their own, beside a binding table of their own (mod_extraction_amd/_hip.py: HEAD_SIGNATURES), because the text of
 * modex_hip.h and _hip.SIGNATURES are held to each other and to a fixed count by the suite.  mx_abi_version() is that of
 * modex_hip.h: entry points are only added. */
#ifndef MODEX_FX_HEAD_H
#define MODEX_FX_HEAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- K17: effect parameters per clip, from a linear head on the extractor's latent (csrc/fx_head.hip) -- no counterpart in
 * the reference.  The table, the slots, the kinds, raw_gain, row_kind and the sample counts are those of K16 (modex_hip.h);
 * raw is no longer shared but one row per clip:
 *   pooled[b, c] = mean_w latent[b, c, w];  raw[b, e] = bias[e] + sum_c weight[e, c] pooled[b, c];  value[b, e] = map(raw[b, e]),
 * each an fp64 evaluation in a fixed order of the fp32 result before it, rounded to fp32 once.  So weight == 0 writes the
 * bits mx_fx_params_expand writes for raw = bias.  latent (B, C, W) fp32 dense, weight (P, C), bias (P,) fp32.  NULL required
 * pointer, P, B, C or W <= 0: MX_ERR_ARG; P > 16, C > 1024 or C W >= 2^31: MX_ERR_UNSUPPORTED; all before any launch.
 *
 * mx_fx_head_fwd (one workgroup per clip): writes pooled (B, C), raw_rows (B, P) (both required: the backward reads them) and
 * values (B, P) (optional), and on the rows of an entry's kind the value into the row of its slot's (B,) vector by the rule
 * of mx_fx_params_expand (lfo_scale / min_delay times the row's sample count in fp32, one_minus_mix = 1 - mix in fp32).  Rows
 * and slots without an entry are not written; a NULL vector skips its slot. */
int mx_fx_head_fwd(const float *latent, int64_t B, int64_t C, int64_t W, const float *weight, const float *bias,
                   const double *tab_f, const int32_t *tab_i, int64_t P, double raw_gain, const int32_t *row_kind,
                   const float *max_lfo_delay, const float *max_min_delay, float *lfo_scale, float *min_delay, float *feedback,
                   float *depth, float *mix, float *one_minus_mix, float *centre_frequency_hz, float *pooled, float *raw_rows,
                   float *values, void *stream);
/* With d_raw[b, e] = scale * grads[slot_e, b] * (the row's sample count where the slot has one) * d value / d raw at
 * raw_rows[b, e] on the rows of the entry's kind, 0 elsewhere (grads (6, B) fp64 as in mx_fx_params_grad; other rows are not
 * read and may hold anything): d_raw_rows (B, P), d_bias (P,) = sum_b d_raw, d_weight (P, C) = sum_b d_raw[b, e] pooled[b, c],
 * d_latent (B, C, W) = (1 / W) sum_e d_raw[b, e] weight[e, c] for every w (every element is written; rows without an entry
 * get exact zeros).  Each output is fp32, optional, and one rounding of an fp64 sum in a fixed order.  At most two launches,
 * no atomics, no workspace: deterministic.  Both count vectors are required. */
int mx_fx_head_bwd(const double *grads, const float *raw_rows, const float *pooled, const float *weight, const double *tab_f,
                   const int32_t *tab_i, int64_t P, double raw_gain, const int32_t *row_kind, const float *max_lfo_delay,
                   const float *max_min_delay, int64_t B, int64_t C, int64_t W, double scale, float *d_raw_rows, float *d_bias,
                   float *d_weight, float *d_latent, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_FX_HEAD_H */
