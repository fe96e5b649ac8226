/* rate_track_abi.h -- the C ABI of K25 (csrc/rate_track.hip): the rate CONTOUR of an LFO track whose rate moves.
 *
 * The conventions are those of include/modex_hip.h (status codes, pointer and scalar kinds, `stream`); the declarations live
 * here, and not there, until they are folded into that header together with an ABI number.  rate_track.hip includes this file,
 * so every definition is compiled against its declaration; mod_extraction_amd/_hip.py derives a fourth ctypes table
 * (SIGNATURES_RATE) from this text.  common.h does not include it.
 *
 * The function.  y: B rows of n fp32 points, y_stride floats apart; sr the rate of the points; starts (S,) int64 on the device,
 * ascending, 0 <= starts[s] <= n - W (a value outside is clamped into that range by every kernel that reads it, so no read
 * leaves the row); W the slice length; [f_min, f_max], shape_mask, rate_div, J, L as in mx_lfo_fit (K18); D the largest rate
 * step between neighbouring slices in grid bins; rate_weight, phase_weight fp64.
 * 1. Node costs.  Slice s of row b is the W points from starts[s].  Its candidates are exactly K18's on a row of n = W: the grid
 *    f_k = f_min + k df, df = sr / (rate_div W), K = floor((f_max - f_min) / df) + 1, phi_j = j 2 pi / J, candidate index
 *    c = k J + j; templates through fit_candidate / lfo_value (lfo_fit_common.h / lfo_common.h); the objective is fit_objective
 *    on centred fp64 slice sums taken in ascending i.  node[sh, s, c] = R / Syy_s, or 0 for every c where Syy_s == 0.
 * 2. Transition from candidate a = (k_a, j_a) of slice s - 1 to b = (k_b, j_b) of slice s: allowed iff |k_b - k_a| <= D;
 *      adv = ((0.5 (f_a + f_b)) (starts[s] - starts[s - 1])) / sr      cycles (the rectified cosines also advance f / sr a point)
 *      m   = ((j_b - j_a) q) / J - adv,  q = 2 for the two rectified cosines (period pi in their own argument), 1 otherwise
 *      m   = m - rint(m);    tr = rate_weight (k_b - k_a)^2 + phase_weight (m m)
 *    in fp64, every product, quotient and sum rounded on its own in the order written (the integer products are exact).
 * 3. Path per (row, shape): V_0[c] = node[0, c];  V_s[b] = node[s, b] + min_a (V_{s-1}[a] + tr(a, b)), ties to the lowest a;
 *    the end is the argmin of V_{S-1}, ties to the lowest c; then backtrack.  The row's shape is the allowed shape of least
 *    total cost, ties to the lowest id.
 * 4. Refinement per slice, on the row's shape only: R0 is the objective at the path's (f_k, phi_j) (sums in ascending i), and
 *    K18's rounds l = 1 .. L (5 x 5 points, a point replacing the best only when strictly smaller: fit_stage) start there; then
 *    amp, offset, resid at the winner as K18's wave 0 forms them.  A constant slice keeps the path's grid candidate: amp 0, offset
 *    its mean, resid 0.
 * Outputs, each one fp32 rounding of the fp64 quantity as in K18: shape (B,) int32; grid_k, grid_j (B, S) int32, the path;
 * rate_hz, phase, amp, offset, resid (B, S) fp32 -- offset + amp * mx_lfo_synth(rate_hz, phase, shape) on W points is the slice's
 * template bit for bit; cost (B,) and per_shape_cost (B, 7) fp32 (+inf where not allowed), the total path costs.
 * With S = 1 the path is the coarse argmin.  The outputs are then mx_lfo_fit's on that slice wherever K18 itself takes its coarse
 * sums in ascending i (K J > 512) and picks, after refinement, the shape the coarse grid picks (always so with one shape).
 *
 * Limits (MX_ERR_UNSUPPORTED): MX_RATE_TRACK_MIN_W <= W <= MX_RATE_TRACK_MAX_W; 1 <= S <= MX_RATE_TRACK_MAX_S;
 * K J <= MX_RATE_TRACK_MAX_STATES (the path keeps a column of V in LDS, 64 KB); 0 <= D <= MX_RATE_TRACK_MAX_D; J in [4, 128],
 * L <= 8, rate_div in [1, 16] as in K18; n <= 2^20; B <= 65535 rows a call.
 * Launches, all on `stream`:
 *   mx_rate_track_nodes    (i) a pre-pass, one 1024-thread workgroup per (slice, row): mean and Syy of the slice in K18's order
 *                          (lanes by butterfly, then the 16 waves in order), to the workspace; (ii) the node launch on
 *                          (candidate tile x shape, slice, row), MX_RATE_TRACK_CAND_TILE candidates a workgroup, one a lane, the
 *                          centred fp64 slice staged in LDS once (8 W bytes), three fp64 sums in ascending i;
 *   mx_rate_track_path     (i) one 1024-thread workgroup per (shape, row) walks the slices in order, lanes over the target states,
 *                          each scanning its (2 D + 1) J allowed sources in ascending a; the column before is in LDS, the int32
 *                          back-pointers go to the workspace; (ii) per row: the argmin over the shapes and the backtrack;
 *   mx_rate_track_refine   one 1024-thread workgroup per (slice, row).
 * No atomics; every sum and every argmin in an order fixed by the arguments, so the same arguments give the same bits.  Every
 * workspace word that is read was written by an earlier launch of the same call sequence (nodes, path, refine, with one
 * workspace and one node table); masked shapes are skipped by the writer and the reader alike; every output is overwritten. */
#ifndef MODEX_RATE_TRACK_ABI_H
#define MODEX_RATE_TRACK_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_RATE_TRACK_MIN_W 16
#define MX_RATE_TRACK_MAX_W 4096
#define MX_RATE_TRACK_MAX_S 16384
#define MX_RATE_TRACK_MAX_STATES 8192
#define MX_RATE_TRACK_MAX_D 16
#define MX_RATE_TRACK_MAX_N 1048576
#define MX_RATE_TRACK_MAX_ROWS 65535
#define MX_RATE_TRACK_CAND_TILE 256

/* The grid and the buffers of a call: *K (the number of rates), *node_bytes (the node table: (B, 7, S, K J) fp64) and *ws_bytes,
 * all HOST int64.  No device work.  The checks every entry point makes after its pointers, in this order:
 * B <= 0: MX_ERR_ARG;  f_min <= 0, f_max < f_min, f_max >= sr / 2, an empty mask or bits above 6, L < 0: MX_ERR_ARG;
 * W, J, L, rate_div, n, B, S or D outside the limits above: MX_ERR_UNSUPPORTED;  n < W: MX_ERR_ARG;  K J too large:
 * MX_ERR_UNSUPPORTED.  A refused plan writes nothing. */
int mx_rate_track_plan(int64_t B, int64_t n, float sr, int64_t S, int64_t W, float f_min, float f_max, int32_t shape_mask,
                       int32_t rate_div, int32_t J, int32_t L, int32_t D, int64_t *K, int64_t *node_bytes, int64_t *ws_bytes);

/* Stage 1.  node: the caller's table, at least node_bytes; ws: at least ws_bytes, both 16-byte aligned device memory (a smaller
 * size or another alignment: MX_ERR_ARG).  NULL y, starts, node or ws, then the checks of the plan (with y_stride < n where
 * mx_lfo_fit checks it), then the buffers; all before any launch. */
int mx_rate_track_nodes(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, const int64_t *starts, int64_t S,
                        int64_t W, float f_min, float f_max, int32_t shape_mask, int32_t rate_div, int32_t J, double *node,
                        int64_t node_bytes, void *ws, int64_t ws_bytes, void *stream);

/* Stages 2 and 3 on the node table mx_rate_track_nodes filled.  rate_weight, phase_weight: finite and >= 0 (else MX_ERR_ARG,
 * after the plan's checks).  Outputs: shape (B,), grid_k, grid_j (B, S) int32; cost (B,), per_shape_cost (B, 7) fp32. */
int mx_rate_track_path(int64_t B, int64_t n, float sr, const int64_t *starts, int64_t S, int64_t W, float f_min, float f_max,
                       int32_t shape_mask, int32_t rate_div, int32_t J, int32_t D, double rate_weight, double phase_weight,
                       const double *node, int64_t node_bytes, void *ws, int64_t ws_bytes, int32_t *shape, int32_t *grid_k,
                       int32_t *grid_j, float *cost, float *per_shape_cost, void *stream);

/* Stage 4 from the path mx_rate_track_path wrote (shape, grid_k, grid_j are inputs here) and the slice statistics
 * mx_rate_track_nodes left in ws.  Outputs (B, S) fp32. */
int mx_rate_track_refine(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, const int64_t *starts, int64_t S,
                         int64_t W, float f_min, float f_max, int32_t shape_mask, int32_t rate_div, int32_t J, int32_t L,
                         const int32_t *shape, const int32_t *grid_k, const int32_t *grid_j, float *rate_hz, float *phase,
                         float *amp, float *offset, float *resid, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_RATE_TRACK_ABI_H */
