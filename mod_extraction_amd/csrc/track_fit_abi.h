/* track_fit_abi.h -- the C ABI of K23 (csrc/track_fit.hip): mx_lfo_fit's function for rows and grids of any length.
 *
 * The conventions are those of include/modex_hip.h (status codes, pointer and scalar kinds, `stream`); the declarations live
 * here, and not there, until they are folded into that header together with an ABI number.  track_fit.hip includes this file,
 * so every definition is compiled against its declaration; mod_extraction_amd/_hip.py derives a second ctypes table
 * (SIGNATURES_TRACK) from this text.  common.h does not include it.
 *
 * Both entry points compute what mx_lfo_fit (K18, modex_hip.h) defines: the same candidates, templates, objective, coarse
 * grid, refinement rounds, ties, constant-row rule, outputs and optional (B, 7) table.  The limits differ:
 *   16 <= n <= MX_TRACK_FIT_MAX_N points;  K = floor((f_max - f_min) / df) + 1 <= MX_TRACK_FIT_MAX_K rates with K J < 2^31,
 *   df = 1 / (rate_div (n / sr)) in fp64 on the fp32 arguments;  J in [4, 128], L <= 8, rate_div in [1, 16] as in K18;  any B.
 * Four launches per 65535 rows, enqueued on `stream`, with a workspace of the caller's (device memory, 16-byte aligned):
 *   1. per row: mean and Syy in fp64 in a fixed order; the centred row yc (fp64) goes to the workspace;
 *   2. the coarse grid on (candidate tile, shape, row): one candidate a lane, MX_TRACK_FIT_CAND_TILE candidates a workgroup,
 *      yc staged through LDS MX_TRACK_FIT_ROW_TILE points at a time, the three sums in ascending i; one (R, c) argmin a
 *      workgroup goes to the workspace;
 *   3. per (shape, row): the argmin over the tiles, then the L refinement rounds as K18 runs them;
 *   4. per row: the argmin over the shapes; amp, offset and resid at the winner.
 * No atomics; every sum in an order that depends on the arguments alone, so the same arguments give the same bits.  Every
 * workspace word that is read was written by an earlier launch of the same call, and every output is overwritten. */
#ifndef MODEX_TRACK_FIT_ABI_H
#define MODEX_TRACK_FIT_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_TRACK_FIT_MAX_N (1 << 20)
#define MX_TRACK_FIT_MAX_K (1 << 20)
#define MX_TRACK_FIT_ROW_TILE 2048
#define MX_TRACK_FIT_CAND_TILE 256

/* The grid and the workspace of a call: *K (the number of rates) and *ws_bytes, both HOST int64.  No device work.
 * NULL K or ws_bytes, B <= 0, f_min <= 0, f_max < f_min, f_max >= sr / 2, an empty mask or bits above 6, L < 0: MX_ERR_ARG;
 * n, J, L, rate_div or K outside the limits above: MX_ERR_UNSUPPORTED; checked in mx_lfo_fit's order. */
int mx_track_fit_plan(int64_t B, int64_t n, float sr, float f_min, float f_max, int32_t shape_mask, int32_t rate_div, int32_t J,
                      int32_t L, int64_t *K, int64_t *ws_bytes);

/* The fit.  Arguments and outputs as mx_lfo_fit; ws: at least the ws_bytes mx_track_fit_plan reports for the same arguments
 * (ws_bytes: what the caller holds; nothing behind the reported size is touched).  The checks of mx_track_fit_plan in the same
 * order, a NULL required pointer (y, the six outputs, ws) among the first and y_stride < n where mx_lfo_fit checks it; then
 * ws not 16-byte aligned or ws_bytes too small: MX_ERR_ARG; all before any launch. */
int mx_track_fit(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, float f_min, float f_max, int32_t shape_mask,
                 int32_t rate_div, int32_t J, int32_t L, int32_t *shape, float *rate_hz, float *phase, float *amp, float *offset,
                 float *resid, float *per_shape_resid, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_TRACK_FIT_ABI_H */
