/*
 * modex_hip.h -- C ABI of libmodex_hip.so: the MI355X (gfx950) kernels behind the
 * mod_extraction hot path.
 *
 * The reference (christhetree/mod_extraction) is pure Python and has no FFI of its own; the
 * boundary a maintainer binds is this flat C ABI, called from the Python classes that mirror the
 * reference's modules (see INTEGRATION.md for the ctypes stub).  Conventions:
 *
 *   - every pointer is a DEVICE pointer borrowed from the caller (torch tensor .data_ptr());
 *     nothing is allocated, freed or retained by the library; no caller-observable global state
 *   - tensors are dense, row-major, float32 unless stated otherwise
 *   - `stream` is a hipStream_t (0 / NULL = default stream); calls are asynchronous and
 *     re-entrant per stream; the library never synchronises
 *   - return value: 0 = launched, MX_ERR_ARG (-1) bad argument, MX_ERR_UNSUPPORTED (-2) size not
 *     supported (e.g. delay line > LDS), MX_ERR_LAUNCH (-3) HIP launch error.  Never throws.
 *   - every entry point is `int mx_name(...)`; a parameter is a pointer or one of int64_t, int32_t, uint64_t,
 *     uint32_t, float, double.  This file is the one statement of the signatures: csrc/common.h includes it, so
 *     the compiler holds every definition to its declaration, and mod_extraction_amd/_hip.py derives its ctypes
 *     table from this text (and refuses any other parameter type).
 *
 * Each entry point cites the reference code it replaces (file:line in /root/reference).
 */
#ifndef MODEX_HIP_H
#define MODEX_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MX_OK 0
#define MX_ERR_ARG (-1)
#define MX_ERR_UNSUPPORTED (-2)
#define MX_ERR_LAUNCH (-3)

/* ABI version, bumped on any signature change. */
int mx_abi_version(void);
/* The library keeps no caller-observable mutable state: every entry point is a function of its arguments and its stream.
 * (Internally: per-device latches of the dynamic-LDS function attribute, and kernel-variant knobs read once from MODEX_*
 * environment variables; neither changes a result.) */

/* ---- K1: LFO synthesis -- mod_extraction/modulations.py:16-57 (make_mod_signal) -------------
 * One row per LFO.  freq, phase, exp: (B,) float32; shape: (B,) int32 in
 * {0 cos, 1 rect_cos, 2 inv_rect_cos, 3 tri, 4 saw, 5 rsaw, 6 sqr} (NULL = cos); exp NULL = 1;
 * start: (B,) int32 sample offset into a longer signal (NULL = 0; datasets.py:442-449 crops the
 * phaser ground truth that way).  The signal has n_src points at rate sr; if n_out != n_src it
 * is resampled with util.py:15-29 (linear, align_corners=True).  out: (B, n_out). */
int mx_lfo_synth(const float *freq, const float *phase, const int32_t *shape, const float *exp,
                 const int32_t *start, int64_t B, int64_t n_src, int64_t n_out, float sr,
                 float *out, void *stream);

/* Synthetic dry audio of the benchmark / test batches (no reference counterpart: the reference trains on recorded
 * guitar): uniform noise in [lo, hi), Philox-4x32-10 keyed by (seed; sample, clip, counter).  Row of clip b at out + b * stride;
 * rows: optional list of n_rows clip indices (NULL = 0 .. n_rows - 1); length of a row = (lens ? lens[clip] : 0) + len_add,
 * at most max_len. */
int mx_uniform_rows(float *out, int64_t stride, const int32_t *rows, int64_t n_rows, const int32_t *lens, int64_t len_add,
                    int64_t max_len, uint64_t seed, uint32_t counter, float lo, float hi, void *stream);

/* ---- util.py:15-29 (linear_interpolate_last_dim, align_corners=True): (rows,n_in)->(rows,n_out) */
int mx_interp_linear(const float *x, int64_t rows, int64_t n_in, int64_t n_out, float *y,
                     void *stream);

/* Transpose of mx_interp_linear restricted to a window of the output axis: dy (rows, j_len) = d loss / d y[:, j0 : j0 + j_len]
 * (zero elsewhere) -> dx (rows, n_in).  Used by an UNFROZEN LFO model inside the TBPTT step (mod_extraction/lightning.py:
 * 361-366: each step back-propagates through its own chunk of the resampled LFO).  Deterministic gather, no atomics. */
int mx_interp_linear_bwd(const float *dy, int64_t dy_stride, int64_t rows, int64_t n_in, int64_t n_out, int64_t j0,
                         int64_t j_len, float *dx, void *stream);

/* ---- K2: flanger / chorus -- mod_extraction/fx.py:72-119 (MonoFlangerChorusModule.apply_effect)
 * x: mono clips, row b at x + b*x_stride (N samples each; x_stride = N for a dense (B,N) tensor);
 * mod (B,n_mod), n_mod == N or shorter (resampled in-kernel).
 * Per-clip float32 constants, each (B,):
 *   lfo_scale     = max_lfo_delay_samples * width            (fx.py:99)
 *   min_delay     = min_delay_width * max_min_delay_samples  (fx.py:98)
 *   feedback, depth, mix, one_minus_mix                      (fx.py:114-117)
 * max_delay (B,) int32: delay-line length M per clip (fx.py:42), max_delay_max = max over the
 * batch.  The delay line lives in LDS: max_delay_max (+ n_mod when the LFO is resampled in-kernel) <= 34784 floats
 * (FL_MAX_M = the CU's 160 KB minus the 24.7 KB record ring of eight 64-sample rows per chunk; it was 37872 with four
 * rows per chunk) = 789 ms at 44.1 kHz -- the shipped configs need 11 ms (flanger) / 40 ms (chorus); longer lines
 * return MX_ERR_UNSUPPORTED.   rows/n_rows: optional subset of clip indices to process (NULL = all B).
 * y: row b at y + b*y_stride, N samples, clipped to [-1,1].  Optional (NULL to skip): mod_up (B,N) resampled LFO,
 * dbg_prev (B,N) int64 and dbg_frac (B,N) = prev_idx_all / delay_read_fraction_all of
 * fx.py:101-102 for index-parity tests. */
int mx_flanger_fwd(const float *x, int64_t x_stride, const float *mod, int64_t n_mod, const float *lfo_scale,
                   const float *min_delay, const float *feedback, const float *depth,
                   const float *mix, const float *one_minus_mix, const int32_t *max_delay,
                   int32_t max_delay_max, const int32_t *rows, int64_t n_rows, int64_t B, int64_t N,
                   float *y, int64_t y_stride, float *mod_up, int64_t *dbg_prev, float *dbg_frac, void *stream);
/* Measurement twin of mx_flanger_fwd (bench.py, SURVEY.md section 8d "measured serial floor"): the same launch with NO
 * global-memory traffic inside the sample loop (constant inputs, only the last chunk stored), i.e. the kernel's
 * dependent chain alone.  Outputs are meaningless; never called by the product.  No reference counterpart. */
int mx_flanger_fwd_probe(const float *x, int64_t x_stride, const float *mod, int64_t n_mod, const float *lfo_scale,
                   const float *min_delay, const float *feedback, const float *depth,
                   const float *mix, const float *one_minus_mix, const int32_t *max_delay,
                   int32_t max_delay_max, const int32_t *rows, int64_t n_rows, int64_t B, int64_t N,
                   float *y, int64_t y_stride, float *mod_up, int64_t *dbg_prev, float *dbg_frac, void *stream);

/* Forward of the flanger adjoint -- fx.py:72-119: mx_flanger_fwd (y bit-identical) that also writes the interpolated tap
 * v[n] of fx.py:113 of every sample to stash (B,N), dense rows (row b at stash + b*N).  mod (B,n_mod) as in mx_flanger_fwd:
 * full rate (adjoint: mx_flanger_bwd) or any 1 <= n_mod < N, resampled in-kernel (adjoint: mx_flanger_bwd_lr); n_mod > N
 * returns MX_ERR_ARG.  Other arguments, limits (the LDS budget includes the n_mod floats of a resampled row) and the rows
 * subset as mx_flanger_fwd. */
int mx_flanger_fwd_stash(const float *x, int64_t x_stride, const float *mod, int64_t n_mod, const float *lfo_scale,
                         const float *min_delay, const float *feedback, const float *depth,
                         const float *mix, const float *one_minus_mix, const int32_t *max_delay,
                         int32_t max_delay_max, const int32_t *rows, int64_t n_rows, int64_t B, int64_t N,
                         float *y, int64_t y_stride, float *stash, void *stream);
/* Adjoint of fx.py:72-119 (the reference's own autograd fails there: its loop writes into delay_buf after gather saved it).
 * The derivative of the loop restated without in-place writes: floor / prev / next have zero derivative, the read
 * fraction and % derivative 1, clip passes the gradient on [-1, 1] inclusive, never-written slots read 0.
 * dy (B,N) row stride dy_stride; x as in the forward; mod (B,N) full rate and stash (B,N) from mx_flanger_fwd_stash, dense
 * rows; per-clip constants, max_delay, max_delay_max, rows / n_rows as mx_flanger_fwd.  ws: (B,N) floats of workspace.
 * Outputs, each optional (NULL skips it): dx, dmod (B,N) with row strides dx_stride / dmod_stride; per-clip fp64
 * d_lfo_scale, d_min_delay, d_feedback, d_depth, d_mix (B,) (d_mix includes the one_minus_mix = 1 - mix path).
 * Deterministic: no float atomics whose order depends on arrival; per-clip sums in fp64 in a fixed order. */
int mx_flanger_bwd(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, const float *mod,
                   const float *stash, const float *lfo_scale, const float *min_delay, const float *feedback,
                   const float *depth, const float *mix, const float *one_minus_mix, const int32_t *max_delay,
                   int32_t max_delay_max, const int32_t *rows, int64_t n_rows, int64_t B, int64_t N,
                   float *ws, float *dx, int64_t dx_stride, float *dmod, int64_t dmod_stride,
                   double *d_lfo_scale, double *d_min_delay, double *d_feedback, double *d_depth,
                   double *d_mix, void *stream);
/* mx_flanger_bwd for the LFO row the data path renders from -- fx.py:72-119 behind the align_corners=True resampling of
 * mod_extraction/util.py:15-29 (linear_interpolate_last_dim, as data_modules.py:455 applies it to the n_samples // 100
 * label before fx.py sees it).  mod (B,n_mod), 1 <= n_mod <= N, is the row mx_flanger_fwd_stash was given; every sample's
 * LFO value is recomputed with the forward's own taps and rounding, so slots and fractions are the forward's.  dmod
 * (B,n_mod), row stride dmod_stride >= n_mod: the transpose of that resampling applied to the per-sample gradient (each
 * rounded to fp32 once, in ws), one fp64 gather per low-rate point over its contiguous range of samples in a fixed order,
 * rounded once -- no atomics, no second (B,N) buffer.  d_lfo_scale uses the resampled values.  n_mod == N is
 * mx_flanger_bwd.  The LDS of the recurrence holds max_delay_max + n_mod floats beside the ring: above FL_MAX_M (34784)
 * it returns MX_ERR_UNSUPPORTED.  Everything else as mx_flanger_bwd. */
int mx_flanger_bwd_lr(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, const float *mod,
                      int64_t n_mod, const float *stash, const float *lfo_scale, const float *min_delay,
                      const float *feedback, const float *depth, const float *mix, const float *one_minus_mix,
                      const int32_t *max_delay, int32_t max_delay_max, const int32_t *rows, int64_t n_rows,
                      int64_t B, int64_t N, float *ws, float *dx, int64_t dx_stride, float *dmod,
                      int64_t dmod_stride, double *d_lfo_scale, double *d_min_delay, double *d_feedback,
                      double *d_depth, double *d_mix, void *stream);

/* Measurement aid (bench.py): `steps` dependent LDS round trips of the flanger lock-step's shape (two ds_read_b32 of the
 * slot the previous step wrote, the five fp32 operations of fx.py:113-115, one ds_write_b32) on one wavefront, nothing
 * else.  Its time per step x the lock-steps of a clip is a floor of mx_flanger_fwd that does not come from that kernel.
 * out: 1 float.  No reference counterpart. */
int mx_lds_roundtrip_probe(int64_t steps, float *out, void *stream);

/* ---- K2c: tremolo -- mod_extraction/fx.py:13-22 (apply_tremolo), one row per (clip, channel):
 *   y[n] = ((1 - mix) * x[n]) + ((mix * m[n]) * x[n]), every operation rounded to fp32 where the reference's torch ops round.
 * x: row b at x + b*x_stride (N samples); y likewise with y_stride.  mod (B,n_mod) dense fp32, 1 <= n_mod <= N: m = mod[n]
 * for n_mod == N, otherwise the row is resampled in-kernel with the align_corners=True rule of util.py:15-29 (the taps and
 * rounding of mx_interp_linear and of mx_flanger_fwd's in-kernel LFO), so the result is bit-identical to resampling first.
 * mix, one_minus_mix (B,) fp32 (both: a python-float mix rounds 1 - mix in double before fp32); rows/n_rows: optional list of
 * rows to process, the others are not touched.  Rows whose pointers are 16-byte aligned move float4s, others single floats.
 * N >= 2^30 returns MX_ERR_UNSUPPORTED. */
int mx_tremolo_fwd(const float *x, int64_t x_stride, const float *mod, int64_t n_mod, const float *mix,
                   const float *one_minus_mix, const int32_t *rows, int64_t n_rows, int64_t B, int64_t N,
                   float *y, int64_t y_stride, void *stream);
/* Adjoint of fx.py:13-22 behind the resampling of util.py:15-29; m is recomputed exactly as in mx_tremolo_fwd (no stash).
 * dy, x: views as above; mod, n_mod, mix, one_minus_mix, rows as the forward was given.  Optional outputs (NULL = skip):
 *   dx    row b at dx + b*dx_stride: dy * (one_minus_mix + mix * m), fp32;
 *   dmod  (B,n_mod) fp32 dense: mix * sum_n w_k(n) dy[n] x[n] with the fp32 tap weights w_k(n) of the resampling, products
 *         and sums in fp64 over the contiguous range of samples with a tap on point k, in a fixed order, rounded once
 *         (n_mod == N: mix * dy * x); no atomics, no workspace: two calls are bit-identical;
 *   dmix  (B,) fp64: sum_n dy x (m - 1), the one_minus_mix path included (the convention of mx_flanger_bwd's d_mix). */
int mx_tremolo_bwd(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, const float *mod,
                   int64_t n_mod, const float *mix, const float *one_minus_mix, const int32_t *rows,
                   int64_t n_rows, int64_t B, int64_t N, float *dx, int64_t dx_stride, float *dmod, double *dmix,
                   void *stream);

/* ---- K3: phaser -- call site mod_extraction/datasets.py:455-482 (pedalboard==0.7.3 Phaser = JUCE
 * dsp::Phaser<float>: 6 first-order TPT all-pass stages + feedback, sine LFO at sr/4 on a log
 * frequency axis, linear dry/wet mix), then clip to [-1,1] (datasets.py:472).  Third-party
 * algorithm restated from its published source: parity unpinned.
 * x: source audio, row b at x + b*x_stride holding lead[b] + N samples; rate, depth, centre,
 * feedback, mix (B,) fp32; lead (B,) int32 = samples rendered before the output window (the
 * reference renders n + sr/rate samples and crops at a random offset, datasets.py:428-449), NULL = 0;
 * rows/n_rows: optional subset of clips.  y: row b at y + b*y_stride = processed[lead:lead+N];
 * dry_out (optional, same stride): the matching crop of x.  exact_order != 0: every sample in JUCE's operation order on
 * one wavefront per clip (the bit reference); 0: the same recurrence as a linear scan over time (512 chunks per clip run
 * in parallel, their affine maps chained; results within 1e-6).  workspace (optional): floats, row i of the processed
 * clips at workspace + i * workspace_stride, >= ceil((lead + N) / 4) each (the cut-off of every 4-sample group, kept
 * between the two passes of the scan; without it the cut-offs are evaluated twice). */
int mx_phaser_fwd(const float *x, int64_t x_stride, const float *rate, const float *depth,
                  const float *centre, const float *feedback, const float *mix, const int32_t *lead,
                  const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, double sr, int32_t exact_order,
                  float *y, int64_t y_stride, float *dry_out, float *workspace, int64_t workspace_stride, void *stream);
/* Measurement twin of mx_phaser_fwd (bench.py, SURVEY.md section 8d "measured serial floor"): the same launch with NO
 * global-memory traffic inside the sample loop (constant inputs, only the last chunk stored), i.e. the kernel's
 * dependent chain alone.  Outputs are meaningless; never called by the product.  No reference counterpart. */
int mx_phaser_fwd_probe(const float *x, int64_t x_stride, const float *rate, const float *depth,
                  const float *centre, const float *feedback, const float *mix, const int32_t *lead,
                  const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, double sr, int32_t exact_order,
                  float *y, int64_t y_stride, float *dry_out, float *workspace, int64_t workspace_stride, void *stream);

/* Forward of the phaser adjoint: the linear scan of mx_phaser_fwd (y and dry_out bit-identical to it when mod is NULL) that
 * can be driven by an external LFO and leaves a stash for mx_phaser_bwd.  x_width: valid floats of a row of x
 * (N <= x_width <= x_stride).  CALLER'S CONTRACT: lead[b] + N <= x_width for every processed clip; lead lives on the device and is
 * not checked by the host: the kernel SKIPS a clip that breaks it -- its y, dry_out and stash rows keep what they held, the
 * status is still MX_OK (fx.phaser_forward_stash asserts the contract).  mod (optional): row b at mod + b*n_mod, one
 * value in [0, 1] per cut-off update (4 samples, from sample 0 of the processed clip), n_mod >= ceil(x_width / 4) (any lead fits):
 * osc = 1 - 2 mod replaces JUCE's sin(phase - pi) = -sin(phase), i.e. mod is the reference's ground-truth LFO
 * make_mod_signal(.., pi / 2, "cos") = (1 + sin wt) / 2 (datasets.py:442, modulations.py:35) sampled every 4th sample; rate is then not read and may be NULL.
 * stash: 16-byte aligned, row b at stash + b*stash_stride, laid out for stash_groups cut-off groups: stash_groups a multiple
 * of 4 and >= ceil(x_width / 4), stash_stride a multiple of 4 and >= 4 stash_groups + 512 * 57 + 512 * 8 * ceil(ceil(stash_groups / 512) / 2) floats
 * (per group G, the lfo before its clamp, osc and the output-clip decisions; per chunk the scan's map; the state at the
 * start of every second group).  Other arguments as mx_phaser_fwd.  No reference counterpart (the reference's phaser is
 * pedalboard's and has no gradient). */
int mx_phaser_fwd_stash(const float *x, int64_t x_stride, int64_t x_width, const float *mod, int64_t n_mod,
                        const float *rate, const float *depth, const float *centre, const float *feedback,
                        const float *mix, const int32_t *lead, const int32_t *rows, int64_t n_rows, int64_t B,
                        int64_t N, double sr, float *y, int64_t y_stride, float *dry_out, float *stash,
                        int64_t stash_groups, int64_t stash_stride, void *stream);
/* Adjoint of the phaser recurrence (oracle_ref.c:orc_phaser): both clips pass the gradient on their closed interval
 * (-1 <= m <= 1, 0 <= lfo <= 1 before clamping: aten's clamp rule).  dy: row b at dy + b*dy_stride, N floats on the output
 * window; x, x_stride, x_width, the parameters, lead, rows / n_rows, B, N, sr and the stash as given to / left by
 * mx_phaser_fwd_stash.  Outputs, each optional (NULL skips it): dx, row b at dx + b*dx_stride, x_width floats: the gradient
 * with respect to EVERY processed source sample, the lead included, zeros beyond lead[b] + N; dmod, row b at
 * dmod + b*dmod_stride, n_mod >= ceil(x_width / 4) floats: the gradient with respect to the external LFO (with the
 * built-in oscillator: with respect to (1 - osc) / 2), zeros beyond the clip's groups; per-clip fp64 d_depth, d_centre
 * (centre_frequency_hz), d_feedback, d_mix (B,).  A clip with lead[b] + N > x_width is skipped as in the forward (outputs
 * untouched, MX_OK; fx.phaser_backward asserts the contract).  No gradient with respect to the rate (see fx.PhaserModule).
 * Deterministic: no atomics; per-clip sums in fp64 in a fixed order. */
int mx_phaser_bwd(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, int64_t x_width,
                  const float *stash, int64_t stash_groups, int64_t stash_stride, const float *depth,
                  const float *centre, const float *feedback, const float *mix, const int32_t *lead,
                  const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, double sr, float *dx,
                  int64_t dx_stride, float *dmod, int64_t dmod_stride, int64_t n_mod, double *d_depth,
                  double *d_centre, double *d_feedback, double *d_mix, void *stream);

/* ---- K3c: the phaser's external LFO at a low rate (the reference has no counterpart: its phaser is pedalboard's, with a
 * built-in oscillator and no gradient).  The linear map from a row of n_mod points spanning the N samples of the clip
 * window (align_corners=True, the resampling of util.py:15-29 as the flanger and tremolo kernels evaluate it) to the
 * cut-off-update grid of mx_phaser_fwd_stash / mx_phaser_bwd, and its transpose.
 * mx_phaser_mod_expand: mod_lr (B, n_mod) fp32 dense, 1 <= n_mod <= N; lead (B,) int32 or NULL (= 0); x_width (>= N): valid
 * floats of a source row, as given to mx_phaser_fwd_stash.  mod_g: row b at mod_g + b*mod_g_stride, mod_g_stride >=
 * ceil(x_width / 4); every one of the ceil(x_width / 4) groups is written: group g < ceil((lead[b] + N) / 4) gets the row
 * resampled at clip sample clamp(4 g - lead[b], 0, N - 1) (held at its first value through the lead-in; n_mod == N: a plain
 * read), the others 0.5. */
int mx_phaser_mod_expand(const float *mod_lr, int64_t n_mod, const int32_t *lead, int64_t B, int64_t N, int64_t x_width,
                         float *mod_g, int64_t mod_g_stride, void *stream);
/* The exact transpose.  dmod_g: row b at dmod_g + b*dmod_g_stride, n_groups valid floats (>= ceil(N / 4)) as mx_phaser_bwd
 * wrote them (its dmod, dmod_stride, n_mod); lead, N, n_mod as given to mx_phaser_mod_expand.  dmod_lr (B, n_mod) fp32 dense:
 * every point is the fp64 sum, in a fixed order, of weight x dmod_g over the groups with a tap on it, rounded once (no
 * atomics: deterministic). */
int mx_phaser_dmod_gather(const float *dmod_g, int64_t dmod_g_stride, int64_t n_groups, const int32_t *lead, int64_t B,
                          int64_t N, int64_t n_mod, float *dmod_lr, void *stream);
/* The two maps on a LIST of rows (the reference has no counterpart): for the phaser clips of a batch that mixes effects, whose
 * LFO rows and gradient rows lie among the other effects' in shared (B, .) buffers.  rows: n_rows int32 clip indices on the
 * device, 1 <= n_rows <= B, in any order; the grid covers n_rows x tiles and a workgroup works on b = rows[blockIdx.x / tiles].
 * Every buffer stays indexed by the full-batch row b (mod_lr + b*n_mod, lead[b], mod_g + b*mod_g_stride, dmod_g +
 * b*dmod_g_stride, dmod_lr + b*n_mod); a row that is not listed is neither read nor written; a listed row holds the bits
 * mx_phaser_mod_expand / mx_phaser_dmod_gather give it (same taps, same fp64 order, one cast; no atomics: deterministic).
 * rows == NULL, n_rows < 1 or n_rows > B: MX_ERR_ARG; the other checks and the grid limits (MX_ERR_UNSUPPORTED) as above, all
 * before any launch.  The indices themselves are device data and are NOT checked by the host: the kernels skip an index
 * outside 0 .. B - 1. */
int mx_phaser_mod_expand_rows(const float *mod_lr, int64_t n_mod, const int32_t *lead, const int32_t *rows, int64_t n_rows,
                              int64_t B, int64_t N, int64_t x_width, float *mod_g, int64_t mod_g_stride, void *stream);
int mx_phaser_dmod_gather_rows(const float *dmod_g, int64_t dmod_g_stride, int64_t n_groups, const int32_t *lead,
                               const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, int64_t n_mod, float *dmod_lr,
                               void *stream);

/* ---- K4: log-mel front end -- mod_extraction/models.py:170-181,199-208
 * (torchaudio MelSpectrogram: n_fft in {512, 1024, 2048} -- every shipped config: 1024 --, hann, centre/reflect, power 2,
 * mel filter bank `fb`; other n_fft: MX_ERR_UNSUPPORTED)
 * x (planes, N), planes = B*in_ch; window (n_fft,); twiddle (n_fft, 2) = exp(-2 pi i m / n_fft);
 * fb (n_fft/2+1, n_mels) row-major; band_lo/band_hi (n_mels,) int32 non-zero row range per mel band.
 * out (planes, n_mels, out_pitch) = log(clip(mel, eps)); out_pitch >= n_frames (352 for 345);
 * columns >= n_frames are zero.  SpecAugment: mel rows [f0,f1) and frames [t0,t1) are set to 0
 * before clip/log (0,0 = no mask).  hop <= 0, n_frames < 0 or n_frames > N/hop + 1 (frames beyond the padded clip):
 * MX_ERR_ARG, before any launch. */
int mx_logmel_fwd(const float *x, int64_t planes, int64_t N, const float *window, const float *twiddle,
                  const float *fb, const int32_t *band_lo, const int32_t *band_hi, int64_t n_fft,
                  int64_t hop, int64_t n_mels, int64_t n_frames, int64_t out_pitch, float eps, int32_t f0,
                  int32_t f1, int32_t t0, int32_t t1, float *out, void *stream);

/* ---- K5/K6: one Spectral2DCNN block -- mod_extraction/models.py:183-195
 * Activation planes are (B, C, H, 352) fp32 (345 valid columns).  Weight packing:
 * flip=0: (Cout,Cin,5,13) -> [ci][kh][kw][co] (forward); flip=1 -> [co][4-kh][12-kw][ci] (dgrad). */
int mx_conv_pack_weights(const float *W, int64_t Cout, int64_t Cin, int32_t flip, float *wt, void *stream);

/* mean / rstd (eps inside the sqrt, biased variance) of f(x) per (b,c) plane over H x Wv;
 * f = PReLU(slope[c]) if slope != NULL else identity.  stats (B, C, 2). */
int mx_plane_stats(const float *x, const float *slope, int64_t B, int64_t C, int64_t H, int64_t Wv,
                   float eps, float *stats, void *stream);
/* The same statistics from the per-row partial sums the f16x3 forward kernels below leave when given slope_out /
 * stats_part: part (B, H, C, 2) = {sum, sum of squares} of PReLU(out) - PReLU(bias_c) over the Wv valid columns of one
 * pooled row (the shift keeps the fp32 row sums free of a common offset: no cancellation for near-constant planes);
 * fp64 across the rows.  bias (C,) / slope (C,): the SAME bias and slope_out the forward kernel was given.
 * The LayerNorm of models.py:186 of the NEXT block without re-reading the plane. */
int mx_plane_stats_finish(const float *part, const float *bias, const float *slope, int64_t B, int64_t C, int64_t H,
                          int64_t Wv, float eps, float *stats, void *stream);

/* LayerNorm -> Conv2d(5x13, dilation (1,dilation), same) -> +bias -> MaxPool(2,1), fused.
 * in (B,Cin,H,352): log-mel (first_layer=1) or the previous block's pooled pre-activations (their
 * PReLU, slope (Cin,), is applied on the fly).  out (B,64,H/2,352) pooled PRE-activations,
 * out_amax (B,64,H/2,352) uint8 = which of the two pooled rows won (first max on ties).
 * Cin: any even number >= 2.  All 352 columns of out and out_amax are written: columns >= Wv of out are zeros, those of
 * out_amax are unspecified (0 or 1).  Columns >= Wv of in are read but never reach a result. */
int mx_conv_block_fwd(const float *in, const float *stats, const float *slope, const float *wt,
                      const float *bias, int64_t B, int64_t Cin, int64_t H, int64_t Wv, int32_t dilation,
                      int32_t first_layer, float *out, uint8_t *out_amax, void *stream);

/* data gradient of the block's convolution: G (B,64,H/2,352) = dL/d(pooled pre-activation),
 * routed through amax; wt_flipped = weights packed with flip=1; dxhat (B,64,H,352).
 * All 352 columns of dxhat are written: columns >= Wv are zeros.  Columns >= Wv of G and amax never reach a result. */
int mx_conv_block_dgrad(const float *G, const uint8_t *amax, const float *wt_flipped, int64_t B, int64_t H,
                        int64_t Wv, int32_t dilation, float *dxhat, void *stream);

/* ---- K6 on the fp16 matrix cores with fp32-equivalent accuracy ("f16x3": every fp32 operand is split into
 * an fp16 pair hi + lo, products are hi*hi + hi*lo + lo*hi accumulated in fp32; 3 MFMAs at 16x the fp32 MFMA
 * rate).  Same reference semantics as mx_conv_block_fwd / mx_conv_block_dgrad (models.py:183-195) for the
 * 64->64 channel blocks.  Operands are prepared once per layer as channels-last fp16 pairs:
 *   w_hi, w_lo : 4*5*13*64*16 halfs each, [cb][kh][kw][khalf][out][8] of weights * 256: the 16 input channels of block cb
 *                lie in two planes of 8, input channel = 16 cb + 8 khalf + j (j = the last index).  flip = 0 (forward):
 *                element = W[co = out][ci = 16 cb + 8 khalf + j][kh][kw] * 256.  flip = 1 (data gradient): the roles of the
 *                channels are exchanged and the taps mirrored, element = W[co = 16 cb + 8 khalf + j][ci = out][4 - kh][12 - kw]
 *                * 256, so that the same kernel computes the transposed convolution
 *   x_hi, x_lo : (B, H, 4, 352, 16) halfs (channel-block major): forward = split of (prelu(x) - mean) * rstd;
 *                dgrad = split of the max-pool routed gradient * S_dz, S_dz = 2^k chosen from max|G|
 *                (scale (2,) device floats receives {S_dz, 1/S_dz}; amax_ws = one uint32 workspace, or with
 *                amax_ready != 0 the bits of max|G| left there by mx_ln_prelu_bwd).  dz_hi = dz_lo = NULL: only the
 *                scale pair is produced (the sparse kernels below take the POOLED operand instead). */
int mx_conv_pack_weights_f16(const float *W, int32_t flip, void *w_hi, void *w_lo, void *stream);
int mx_conv_prep_fwd_f16(const float *x, const float *stats, const float *slope, int64_t B, int64_t H,
                         int64_t Wv, void *x_hi, void *x_lo, void *stream);
int mx_conv_prep_dgrad_f16(const float *G, const uint8_t *amax, int64_t B, int64_t H, int64_t Wv,
                           uint32_t *amax_ws, int32_t amax_ready, float *scale, void *dz_hi, void *dz_lo,
                           void *stream);
/* slope_out (64,) / stats_part (B, H/2, 64, 2), both optional: the PReLU slope that follows this block (models.py:194) and
 * the partial LayerNorm statistics of the next block's input for mx_plane_stats_finish. */
int mx_conv_block_fwd_f16(const void *x_hi, const void *x_lo, const void *w_hi, const void *w_lo,
                          const float *bias, int64_t B, int64_t H, int64_t Wv, int32_t dilation, float *out,
                          uint8_t *out_amax, const float *slope_out, float *stats_part, void *stream);
int mx_conv_block_dgrad_f16(const void *dz_hi, const void *dz_lo, const void *w_hi, const void *w_lo,
                            const float *scale, int64_t B, int64_t H, int64_t Wv, int32_t dilation,
                            float *dxhat, void *stream);
/* First block (2 input channels) on the same matrix-core kernel: (kernel row, input channel) pairs become the 16
 * "channels" of the operand (k = kh*2 + ci, 10 used), so that one 16-deep MFMA k-step covers a tap column and the
 * K loop is a single stage.  Same reference semantics (models.py:183-195, first block: LayerNorm -> Conv2d(2,64,
 * (5,13)) -> +bias -> MaxPool(2,1)).  w_hi, w_lo: 13*2*64*8 halfs each; xk_hi, xk_lo: (B, H, 352, 16) halfs.
 * mx_conv_block1_fwd_f16 writes all 352 columns of out and out_amax: columns >= Wv of out are zeros, those of out_amax
 * are unspecified (0 or 1). */
int mx_conv_pack_weights_kvec_f16(const float *W, void *w_hi, void *w_lo, void *stream);
int mx_conv_prep_fwd_kvec_f16(const float *x, const float *stats, int64_t B, int64_t H, int64_t Wv, void *xk_hi,
                              void *xk_lo, void *stream);
int mx_conv_block1_fwd_f16(const void *xk_hi, const void *xk_lo, const void *w_hi, const void *w_lo, const float *bias,
                           int64_t B, int64_t H, int64_t Wv, float *out, uint8_t *out_amax, const float *slope_out,
                           float *stats_part, void *stream);
/* weight gradient of the first block from the same k-vector operand (torch Conv2d backward w.r.t. weight,
 * models.py:187).  G, amax (B,64,H/2,352): gradient w.r.t. the pooled output and the pooling argmax; amax_bits: bit
 * pattern of max|G| (mx_ln_prelu_bwd's gmax_bits); scale (2,) receives {S, 1/S}; part: workspace of
 * ceil(B*H/rows_per_slab)*13*64*16 floats; dW (64,2,5,13). */
int mx_conv_block1_wgrad_f16(const float *G, const uint8_t *amax, const uint32_t *amax_bits, const void *xk_hi,
                             const void *xk_lo, int64_t B, int64_t H, int64_t Wv, int64_t rows_per_slab, float *scale,
                             float *part, float *dW, void *stream);
/* The same with the gradient handed over as f16x3 PAIRS: Gp (B,64,H/2,352) uint32 = (hi | lo << 16) of G * scale[0] per element
 * (fp16 bit patterns), as mx_ln_prelu_bwd_pair leaves them; scale {S, 1/S} from mx_ln_bwd_finish.  Same reference lines. */
int mx_conv_block1_wgrad_pair_f16(const void *Gp, const uint8_t *amax, const float *scale, const void *xk_hi, const void *xk_lo,
                                  int64_t B, int64_t H, int64_t Wv, int64_t rows_per_slab, float *part, float *dW, void *stream);

/* weight gradient from the same prepared operands (dz pair of mx_conv_prep_dgrad_f16, x pair of
 * mx_conv_prep_fwd_f16); part = workspace of ceil(B*H/rows_per_slab)*65*64*64 floats; dW (64,64,5,13). */
int mx_conv_block_wgrad_f16(const void *dz_hi, const void *dz_lo, const void *x_hi, const void *x_lo,
                            const float *scale, int64_t B, int64_t H, int32_t dilation, int64_t rows_per_slab,
                            float *part, float *dW, void *stream);

/* weight gradient: x (B,Cin,H,352) = block input before PReLU/LayerNorm (Cin = 64, or 2 for the
 * first block with slope = NULL); part = workspace of ceil(B*H/rows_per_slab)*65*64*Cin floats;
 * dW (64,Cin,5,13) torch layout, overwritten. */
int mx_conv_block_wgrad(const float *G, const uint8_t *amax, const float *x, const float *stats,
                        const float *slope, int64_t B, int64_t Cin, int64_t H, int64_t Wv, int32_t dilation,
                        int64_t rows_per_slab, float *part, float *dW, void *stream);

/* The same weight gradient on the SPARSE fp16 matrix instruction (v_smfmac_f32_32x32x32_f16): with K ordered as
 * (position, row of the pooling pair) the routed gradient is 2:4 structured sparse -- its compressed form is the pooled
 * gradient G itself, its index bits are the pooling argmax -- so one instruction covers both rows of a pooling pair
 * (half the matrix instructions of mx_conv_block_wgrad_f16; identical results up to fp32 summation order).
 * g_hi, g_lo (B,H/2,4,352,16) halfs = the channels-last split of G * S and gidx (B,64,H/2,22,2) uint16 index words (word of
 * (k-step ks of 16 positions, lane half hh): field j = 2 gq + e, j = 0..7, in bits [2 j, 2 j + 2) = 2 e + (amax & 1) at
 * position 16 ks + 8 (gq >> 1) + 4 hh + 2 (gq & 1) + e), both
 * from mx_conv_prep_gpool_cl_f16 below (the pair is the operand of the sparse data gradient as well; its [position]
 * [channel] rows become the A fragments through transposing LDS reads).  rows_per_slab counts POOLED rows;
 * Wv <= 351 (MX_ERR_UNSUPPORTED otherwise: the zero pad column of the x operand is the kernel's halo source); H even, >= 2
 * (MX_ERR_UNSUPPORTED otherwise, as mx_conv_block_fwd_f16 and both data gradients);
 * part: ceil(B*(H/2)/rows_per_slab)*65*64*64 floats. */
int mx_conv_block_wgrad_sp_f16(const void *g_hi, const void *g_lo, const void *gidx, const void *x_hi, const void *x_lo,
                               const float *scale, int64_t B, int64_t H, int64_t Wv, int32_t dilation,
                               int64_t rows_per_slab, float *part, float *dW, void *stream);

/* The data gradient on the sparse matrix instruction as well.  The sparse operand must be A, so tiles are computed
 * transposed ([position][ci]) with K = (output channel, row of the pooling pair): compressed A = the pooled gradient
 * in channels-last form, B = the weights of the two kernel rows the pair meets, packed in fragment order and read
 * from global memory; 12 K stages instead of 20.  Same results as mx_conv_block_dgrad_f16 up to summation order.
 *   mx_conv_pack_weights_sp_f16: W (64,64,5,13) -> w_hi, w_lo: 4*3*2*13*2*64*16 halfs each, [cb][m][r][kwf][ci tile][lane][16]
 *                              of weights * 256 in fragment order: for output row h = 2 hp + r the pooling pair hp + m - 1
 *                              (m = 0, 1, 2) and the position w + (kwf - 6) * dilation; lane l holds column n = l & 31 and
 *                              k half s = l >> 5, its element j is k = 16 s + j: output channel co = 16 cb + (k >> 1), row
 *                              of the pair = k & 1, hence kernel row kh = 4 + r - 2 m - (k & 1) (element = 0 where kh is
 *                              outside 0..4), kernel column kw = 12 - kwf, input channel ci = 32 (ci tile) + n:
 *                              element = W[co][ci][kh][kw] * 256
 *   mx_conv_prep_gpool_cl_f16: G, amax (B,64,H/2,352), scale {S, 1/S} -> g_hi, g_lo (B,H/2,4,352,16) halfs,
 *                              g_idx (B,H/2,4,352) uint32 index words of the data gradient: the word of (clip, pooled
 *                              row, channel block cb, position) holds sixteen 2-bit fields, field j (j = 0..7) of lane half
 *                              hf (0, 1) in bits [16 hf + 2 j, 16 hf + 2 j + 2) = 2 (j & 1) + (amax & 1) of output channel
 *                              16 cb + (j < 4 ? 4 hf + j : 8 + 4 hf + j - 4); every one of the 352 positions has a word
 *                              (from amax as it stands there), while g_hi, g_lo are +0 at positions >= Wv; gidx (or NULL):
 *                              (B,64,H/2,22,2) uint16 index words of mx_conv_block_wgrad_sp_f16 from the same pass
 *                              (mx_conv_prep_dgrad_f16 with dz_hi = dz_lo = NULL then only computes the scale pair)
 *   mx_conv_block_dgrad_sp_f16: dxhat (B,64,H,352); Wv <= 351 (zero pad column = halo source).  x_hi, x_lo, ln_part
 *                              (all or NULL): the block's forward operand pair (B,H,4,352,16) = the normalised input
 *                              xhat, and ln_part (B,64,H,2,2) floats <- {sum dxhat, sum dxhat * xhat} per (plane, row,
 *                              position half): the plane statistics mx_ln_prelu_bwd needs, taken while the values are
 *                              in registers instead of by a sweep over dxhat and p.  gx_bits (2 uint32, zeroed by the
 *                              caller; optional, needs ln_part): receives the bit patterns of max|dxhat| and max|xhat|
 *                              of the launch (atomic max) for mx_ln_bwd_finish */
int mx_conv_pack_weights_sp_f16(const float *W, void *w_hi, void *w_lo, void *stream);
int mx_conv_prep_gpool_cl_f16(const float *G, const uint8_t *amax, const float *scale, int64_t B, int64_t H, int64_t Wv,
                              void *g_hi, void *g_lo, void *g_idx, void *gidx, void *stream);
int mx_conv_block_dgrad_sp_f16(const void *g_hi, const void *g_lo, const void *g_idx, const void *w_hi, const void *w_lo,
                               const float *scale, int64_t B, int64_t H, int64_t Wv, int32_t dilation, float *dxhat,
                               const void *x_hi, const void *x_lo, float *ln_part, uint32_t *gx_bits, void *stream);
/* LayerNorm / PReLU backward (torch autograd of models.py:186,194) written STRAIGHT INTO the pooled operand of the block below,
 * for blocks whose two gradients both take the pooled channels-last pair: dL/dp never exists in fp32 (8 B per element less
 * than mx_ln_prelu_bwd + mx_conv_prep_gpool_cl_f16).  The f16x3 scale is needed before the pass, so it comes from an upper
 * bound on max|G| instead of the maximum itself:
 *   mx_ln_bwd_finish: ln_part (B,C,H,2,2), stats (B,C,2), slope (C,), gx_bits (2,) as left by mx_conv_block_dgrad_sp_f16 ->
 *                     m12 (B,C,2) = plane means {dxhat, dxhat * xhat}; scale (2,) = {S, 1/S}, S the power of two that puts
 *                     max_p rstd_p max(1,|slope|) (max|dxhat| + |m1_p| + max|xhat| |m2_p|) into [512, 1024); bound_ws: 1 uint32
 *   mx_ln_prelu_bwd_gpool_f16: p, dxhat, amax (B,64,Hp,352) -> g_hi, g_lo (B,Hp,4,352,16), g_idx (B,Hp,4,352), gidx
 *                     (B,64,Hp,22,2; optional) exactly as mx_conv_prep_gpool_cl_f16 would from G; part: workspace of
 *                     B*64*Hp*6*2 floats; dslope_part, gsum_part (B*64,): the per-plane sums mx_ln_prelu_bwd returns */
int mx_ln_bwd_finish(const float *ln_part, const float *stats, const float *slope, const uint32_t *gx_bits, int64_t B,
                     int64_t C, int64_t H, int64_t Wv, float *m12, uint32_t *bound_ws, float *scale, void *stream);
int mx_ln_prelu_bwd_gpool_f16(const float *p, const float *dxhat, const uint8_t *amax, const float *stats,
                              const float *slope, const float *m12, const float *scale, int64_t B, int64_t Hp, int64_t Wv,
                              void *g_hi, void *g_lo, void *g_idx, void *gidx, float *part, float *dslope_part,
                              float *gsum_part, void *stream);

/* LayerNorm backward fused with the backward of the PReLU in front of it.  p (B,C,H,352): input of
 * that PReLU; dxhat_inout: in = grad w.r.t. the normalised tensor, out = G = dL/dp (in place);
 * dslope_part (B*C,) per-plane partial of dL/dslope.  Optional by-products of the same pass (NULL = skip):
 * gsum_part (B*C,) = per-plane sum of G (the bias gradient partials mx_plane_sum would produce) and
 * gmax_bits: atomicMax of the bit pattern of |G| into one zero-initialised uint32 (the amax_ready input of
 * mx_conv_prep_dgrad_f16).  ln_part (NULL = compute them here): (B,C,H,2,2) partial sums {sum dxhat, sum dxhat *
 * xhat} left by mx_conv_block_dgrad_sp_f16; with them the kernel reads each tensor once instead of twice. */
int mx_ln_prelu_bwd(const float *p, float *dxhat_inout, const float *stats, const float *slope, int64_t B,
                    int64_t C, int64_t H, int64_t Wv, float *dslope_part, float *gsum_part, uint32_t *gmax_bits,
                    const float *ln_part, void *stream);
/* mx_ln_prelu_bwd that leaves G as f16x3 pairs in place: element -> (hi | lo << 16) of G * scale[0] (the operand of
 * mx_conv_block1_wgrad_pair_f16); scale = {S, 1/S} from mx_ln_bwd_finish, ln_part required.  Same reference lines. */
int mx_ln_prelu_bwd_pair(const float *p, float *dxhat_inout, const float *stats, const float *slope, int64_t B, int64_t C,
                         int64_t H, int64_t Wv, float *dslope_part, float *gsum_part, const float *ln_part, const float *scale,
                         void *stream);

/* out[c] (+)= sum_r part[r*C + c]  (fp64 accumulate; deterministic) */
int mx_reduce_rows(const float *part, int64_t R, int64_t C, int32_t accumulate, float *out, void *stream);

/* out[plane] = sum over the H x Wv valid region of each (H,352) plane (bias gradients). */
int mx_plane_sum(const float *x, int64_t planes, int64_t H, int64_t Wv, float *out, void *stream);

/* ---- K7: head -- mod_extraction/models.py:209-215: PReLU -> mean over bins -> Conv1d(C->L,k=1) ->
 * sigmoid.  p6 (B,C,Hl,352); latent (B,C,Wv) and out (B,L,Wv) dense.  L <= 4. */
int mx_head_fwd(const float *p6, const float *slope, const float *wout, const float *bout, int64_t B,
                int64_t C, int64_t Hl, int64_t Wv, int64_t L, float *latent, float *out, void *stream);
/* gmax_bits (optional, zeroed by the caller): receives the bit pattern of max|G6| (atomic max) -- the f16x3 gradient scale of
 * the last block without a sweep over G6 (mx_conv_prep_dgrad_f16 with amax_ready = 1). */
int mx_head_bwd(const float *p6, const float *slope, const float *wout, const float *latent,
                const float *out, const float *d_out, const float *d_latent, int64_t B, int64_t C,
                int64_t Hl, int64_t Wv, int64_t L, float *G6, float *dwout_part, float *dbout_part,
                float *dslope_part, uint32_t *gmax_bits, void *stream);

/* ---- K8: LFO loss -- mod_extraction/lightning.py:33-62 + losses.py:70-102 (l1, fdl1, sdl1, mse,
 * 'mean' reductions).  y_hat, y (B,n), n <= 2048; part (B,4) workspace; losses (5,) = l1, fdl1,
 * sdl1, mse, weighted total (weights <= 0 are logged but not added); grad (B,n) or NULL = d total / d y_hat
 * (so a term with a weight <= 0 is absent from it too). */
int mx_lfo_loss(const float *y_hat, const float *y, int64_t B, int64_t n, float w_l1, float w_fdl1,
                float w_sdl1, float w_mse, float *part, float *losses, float *grad, void *stream);

/* ---- K9: LFO post-processing -- mod_extraction/modulations.py:219-363; all bit-exact fp32.
 * x (rows, n) dense. */
/* smoothen (modulations.py:359-363): out (rows, n-k+1) = moving average over k frames. */
int mx_smoothen(const float *x, int64_t rows, int64_t n, int64_t k, float *out, void *stream);
/* find_corners (modulations.py:219-238): top/bot (rows, n) float maps. */
int mx_find_corners(const float *x, int64_t rows, int64_t n, float *top, float *bot, void *stream);
/* stretch_corners after smoothing (modulations.py:260-307): out (rows, n). */
int mx_stretch_corners(const float *x, int64_t rows, int64_t n, int64_t max_n_corners, float *out,
                       void *stream);
/* Gradient of mx_stretch_corners w.r.t. its input (mod_extraction/modulations.py:260-291 is written with differentiable torch
 * ops; lightning.py:294-296 with an unfrozen LFO model back-propagates through it): x = that call's input, dout = gradient
 * w.r.t. its output -> dx.  Corner positions / targets are discrete and carry no gradient. */
int mx_stretch_corners_bwd(const float *x, const float *dout, int64_t rows, int64_t n, int64_t max_n_corners, float *dx,
                           void *stream);
/* check_mod_sig (modulations.py:311-343) per row: valid (rows,) int32 0/1;
 * min_gap = int(min_fraction_between_corners * n). */
int mx_check_mod_sig(const float *x, int64_t rows, int64_t n, int32_t min_top, int32_t max_top,
                     int32_t min_bot, int32_t max_bot, int32_t min_gap, int32_t *valid, void *stream);

/* ---- K14: evaluation LFO variants for a whole batch -- mod_extraction/modulations.py:104-160 and :191-210 as
 * datasets.py:365-398 applies them per item (fx_config.mod_sig.quasiperiodic / .combined of configs/eval_lfo_quasi.yml and
 * eval_lfo_combined.yml).  The reference draws a data-dependent number of random values per LFO on the host; here the draws
 * arrive as a fixed-width table per row (S entries) that the kernel consumes in corner order.  One launch, one workgroup per
 * row, no host round trip, no atomics, no workspace; bit-identical from run to run.  Limits (MX_ERR_UNSUPPORTED): S in
 * 1 .. 64, n <= 16 777 216 (rows stay in global memory -- LDS holds the corner list and the section table only -- so the bound
 * is the fp32 index arithmetic of the align_corners resampling, exact below 2^24), B < 2^31. */
/* make_quasi_periodic + _time_stretch_section (modulations.py:104-160) on every row of base (B, n), n >= 3.  The corner map
 * with the larger sum is taken (top if its sum EXCEEDS the bottom's, modulations.py:129-132), its entries equal to 1 are the
 * corners c_0 < .. < c_(m-1).  Section s = base[p_s .. c_s] (p_0 = 0, p_s = c_(s-1)), size = c_s - p_s + 1,
 * x = (int)((double)amount[b][s] * size + 0.5), new = shrink[b][s] ? max(2, size - x) : size + x; the section contributes the
 * first new - 1 points of its align_corners resampling to `new` points (util.py:15-29).  The tail base[c_(m-1) .. n-1] is
 * stretched when pieces and tail together fall short of n, and the concatenation is cut to n.  amount >= 0 is expected
 * (amount * size is clamped to +-2^30).  Rows with fewer than 2 corners (modulations.py:136-137) or with more than S corners
 * are copied unchanged.  n_corners (B,) int32 or NULL receives m, the real count, in every case.  out (B, n) must not alias
 * base. */
int mx_lfo_quasi_periodic(const float *base, const int32_t *shrink, const float *amount, int64_t B, int64_t n, int64_t S,
                          float *out, int32_t *n_corners, void *stream);
/* make_combined_mod_sig (modulations.py:191-210) for B rows: freq, phase (B,) float32; shape_tab (B, S + 1) int32 shape ids as
 * in mx_lfo_synth.  Column 0 is the shape of the base LFO, synthesised as mx_lfo_synth does with n_src = n_out = n at rate
 * sr, exponent 1, start 0.  With c_0 < .. < c_(m-1) the bottom corners of the base, points c_s .. c_(s+1) become
 * make_mod_signal(L, L, freq=1, phase=0, shape_tab[b][s + 1]) with L = c_(s+1) - c_s + 1; a shared corner belongs to the
 * later section (the later assignment wins in the reference's loop), the last corner to the last section.  Pairs beyond S
 * keep the base; so does a row with fewer than 2 bottom corners.  n_corners (B,) int32 or NULL receives m.  out (B, n). */
int mx_lfo_combined(const float *freq, const float *phase, const int32_t *shape_tab, int64_t B, int64_t n, int64_t S,
                    float sr, float *out, int32_t *n_corners, void *stream);

/* ---- K10: LSTM-64 effect model -- mod_extraction/models.py:311-339 (nn.LSTM(2,64) -> Linear(64,1) ->
 * + x -> tanh, input order (lfo, audio)) and its truncated BPTT, lightning.py:355-384.
 * x, lfo, y: B rows of T samples with row strides (chunks are views into (B,1,n) tensors).
 * Parameters in torch layout: w_ih (256,2), w_hh (256,64), b_ih (256), b_hh (256), fc_w (64), fc_b (1).
 * h_in, c_in (B,64): state entering the chunk (read only); h_out, c_out (B,64): state leaving it (may alias the
 * inputs when no backward follows: HiddenStateModel.update_hidden, models.py:298-301).  stash (B,T,384) = per-step
 * (i,f,g,o,c,h) for the backward, or NULL. */
int mx_lstm_fwd(const float *x, int64_t x_stride, const float *lfo, int64_t lfo_stride, const float *w_ih,
                const float *w_hh, const float *b_ih, const float *b_hh, const float *fc_w, const float *fc_b,
                const float *h_in, const float *c_in, float *h_out, float *c_out, float *y, int64_t y_stride,
                float *stash, int64_t B, int64_t T, void *stream);
/* Measurement twin of mx_lstm_fwd (bench.py, SURVEY.md section 8d "measured serial floor"): the same launch with NO
 * global-memory traffic inside the sample loop (constant inputs, only the last chunk stored), i.e. the kernel's
 * dependent chain alone.  Outputs are meaningless; never called by the product.  No reference counterpart. */
int mx_lstm_fwd_probe(const float *x, int64_t x_stride, const float *lfo, int64_t lfo_stride, const float *w_ih,
                const float *w_hh, const float *b_ih, const float *b_hh, const float *fc_w, const float *fc_b,
                const float *h_in, const float *c_in, float *h_out, float *c_out, float *y, int64_t y_stride,
                float *stash, int64_t B, int64_t T, void *stream);
/* BPTT of one chunk with nn.L1Loss fused: loss = loss_scale * sum |y - wet| (loss_scale = w/(B*T)).
 * h_init, c_init (B,64): state at the chunk start (detached, lightning.py:383).  part (B,17473):
 * per-clip gradient rows in state-dict order [weight_ih | weight_hh | bias_ih | bias_hh | fc.weight |
 * fc.bias]; sum them with mx_reduce_rows. */
int mx_lstm_bwd_l1(const float *x, int64_t x_stride, const float *lfo, int64_t lfo_stride, const float *y,
                   int64_t y_stride, const float *wet, int64_t wet_stride, const float *stash,
                   const float *w_hh, const float *fc_w, const float *h_init, const float *c_init,
                   float loss_scale, float *part, int64_t B, int64_t T, void *stream);
/* The same BPTT for ANY loss -- mod_extraction/lightning.py:380-382 back-propagates whatever calc_and_log_losses returns
 * (losses.py:142-160): dy (B rows, stride dy_stride) = d loss / d y of every output sample of the chunk, produced by
 * mx_effect_loss_grad (L1 / MSE / ESR / DC), mx_mrstft_loss (dx) or their sum.  Other arguments as mx_lstm_bwd_l1. */
int mx_lstm_bwd(const float *x, int64_t x_stride, const float *lfo, int64_t lfo_stride, const float *y,
                int64_t y_stride, const float *dy, int64_t dy_stride, const float *stash, const float *w_hh,
                const float *fc_w, const float *h_init, const float *c_init, float *part, int64_t B, int64_t T,
                void *stream);
/* Measurement twin of mx_lstm_bwd_l1 (bench.py, SURVEY.md section 8d "measured serial floor"): the same launch with NO
 * global-memory traffic inside the sample loop (constant inputs, only the last chunk stored), i.e. the kernel's
 * dependent chain alone.  Outputs are meaningless; never called by the product.  No reference counterpart. */
int mx_lstm_bwd_l1_probe(const float *x, int64_t x_stride, const float *lfo, int64_t lfo_stride, const float *y,
                   int64_t y_stride, const float *wet, int64_t wet_stride, const float *stash,
                   const float *w_hh, const float *fc_w, const float *h_init, const float *c_init,
                   float loss_scale, float *part, int64_t B, int64_t T, void *stream);

/* mx_lstm_bwd_l1 / mx_lstm_bwd that ALSO leaves the gate gradients dgate (B, T, 256) (row order of weight_ih_l0): wet != NULL
 * selects the fused nn.L1Loss (loss_scale), else dy = d loss / d y.  mx_lstm_dlfo: dlfo[b][t] = sum_r weight_ih[r][0] dgate[b][t][r]
 * = d loss / d lfo of every sample -- mod_extraction/lightning.py:258,344-366 with freeze_lfo_model: false (the LFO model is
 * re-run inside every TBPTT step and trained through the effect model). */
int mx_lstm_bwd_dgate(const float *x, int64_t x_stride, const float *lfo, int64_t lfo_stride, const float *y,
                      int64_t y_stride, const float *wet, int64_t wet_stride, const float *dy, int64_t dy_stride,
                      const float *stash, const float *w_hh, const float *fc_w, const float *h_init, const float *c_init,
                      float loss_scale, float *part, float *dgate, int64_t B, int64_t T, void *stream);
int mx_lstm_dlfo(const float *dgate, const float *w_ih, int64_t B, int64_t T, float *dlfo, int64_t dlfo_stride, void *stream);

/* Measurement aid (bench.py, `frac_of_independent_floor` of the phaser scan): `steps` samples of the bare 6-stage all-pass
 * cascade + feedback (38 flops) for eight independent state vectors per lane -- the shape of the scan's phase A -- on ONE
 * 512-lane workgroup: no loads, stores, cut-off evaluation, chunk maps or chaining.  time / (steps x 8) x ceil((lead + N) / 512)
 * x 9 runs is a floor of mx_phaser_fwd that does not come from that kernel.  out: >= 512 floats.  No reference counterpart. */
int mx_phaser_cascade_probe(int64_t steps, float *out, void *stream);

/* Measurement aid (bench.py, `frac_of_independent_floor` of the LSTM kernels): `steps` dependent recurrent steps of the bare
 * shape of models.py:333 (kind 0: LDS broadcast of h -> 16 packed FMAs -> cross-lane adds -> v_exp / v_rcp gate -> exchange ->
 * cell update -> tanh -> LDS write -> s_barrier) or of its BPTT (kind 1: gate gradients from LDS -> 16 packed FMAs -> all-reduce
 * over 16 row groups -> dh, dc, dg -> LDS write -> s_barrier) on ONE 512-lane workgroup, or (kind 2) the forward step in the
 * 256-lane decomposition that mx_lstm_fwd launches since round 6 (32 packed FMAs per lane, one cross-lane add): no global memory,
 * no input term, no stash, no output layer, no weight gradients.  Time / steps x T is a floor of a T-step launch that does not come from the
 * product kernels.  out: 1 float (keeps the chain live).  No reference counterpart. */
int mx_lstm_step_probe(int32_t kind, int64_t steps, float *out, void *stream);

/* ---- TCN extractors -- mod_extraction/tcn.py:106-302 (TCNBlock / TCN) under models.py:72-125,218-289
 * (SpectralTCN / SpectralDSTCN).  Activations: (B, C, 352) fp32 planes with T <= 352 valid columns.
 * mx_sgemm_f32: general fp32 GEMM on the matrix cores (exact fp32), element strides for every operand:
 *   C[m c_rs + n c_cs] (+)= sum_k A[m a_rs + k a_cs] B[k b_rs + n b_cs], n_batch batches a_bs / b_bs apart;
 *   batches_per_group consecutive batches are summed inside the kernel, group g writes C + g c_bs.
 * mx_tcn_im2col: col[(ci ksz + k)][b To + t'] = xhat[b][ci][t' stride + (k - ksz/2) dilation] (0 outside [0,T));
 *   xhat = (x - stats[2b]) stats[2b+1] (LayerNorm([C,T]) statistics from mx_plane_stats(x, NULL, B, 1, C, T)) or x.
 * mx_tcn_col2im: the transposed gather (gradient w.r.t. xhat).
 * mx_tcn_act_fwd: z += bias (kept: PReLU input); y = PReLU(z) + res.  mx_tcn_act_bwd: dz = dy PReLU'(zb);
 *   part (B*C, 2) = row sums of dz and of dy zb [zb <= 0] (bias / slope gradients after mx_reduce_rows).
 * mx_tcn_ln_bwd: dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) + add, per clip. */
int mx_sgemm_f32(const float *a, int64_t a_rs, int64_t a_cs, int64_t a_bs, const float *b, int64_t b_rs, int64_t b_cs,
                 int64_t b_bs, float *c, int64_t c_rs, int64_t c_cs, int64_t c_bs, int64_t M, int64_t N, int64_t K,
                 int64_t n_batch, int64_t batches_per_group, int32_t accumulate, void *stream);
int mx_tcn_im2col(const float *x, const float *stats, int64_t B, int64_t C, int64_t T, int64_t To, int64_t ksz,
                  int64_t dilation, int64_t stride, float *col, void *stream);
int mx_tcn_col2im(const float *dcol, int64_t B, int64_t C, int64_t T, int64_t To, int64_t ksz, int64_t dilation,
                  int64_t stride, float *dx, void *stream);
int mx_tcn_act_fwd(float *z, const float *bias, const float *slope, const float *res, int64_t B, int64_t C, int64_t T,
                   float *y, void *stream);
int mx_tcn_act_bwd(const float *dy, const float *zb, const float *slope, int64_t B, int64_t C, int64_t T, float *dz,
                   float *part, void *stream);
int mx_tcn_ln_bwd(const float *x, const float *dxhat, const float *stats, const float *add, int64_t B, int64_t C,
                  int64_t T, float *dx, void *stream);

/* ---- Spectral2DCNN outside the 5x13 / 64-channel / pool (2,1) family -- mod_extraction/models.py:127-215 with any kernel
 * size, channel list, dilations, MaxPool2d((p,1)), use_ln, in_ch, frame count and latent_dim (the class's own defaults
 * are such a configuration).  Dense NCHW fp32 tensors, exact fp32 arithmetic; the three convolution products are
 * mx_sgemm_f32 on the matrices these gathers build.
 * mx_im2col2d: col[(ci kh + i) kw + j][(b H + h) W + w] = x[b][ci][h + i dh - pt][w + j dw - pl] (0 outside the image) for
 *   the nb clips at x; "same" padding (models.py:187): pt = dh (kh - 1) / 2, pl = dw (kw - 1) / 2 (aten: the remainder goes
 *   after).  mx_col2im2d: the transposed gather, dx[b][ci][y][x] = sum over taps of dcol[...] (gradient w.r.t. x).
 * mx_rowln_fwd / _bwd: nn.LayerNorm([bins, frames], elementwise_affine=False) (models.py:186) of `rows` contiguous rows of n
 *   elements: y = (x - mean) rstd, stats (rows, 2) = {mean, rstd}; dx = rstd (dy - mean(dy) - y mean(dy y)).
 * mx_pool_prelu_fwd / _bwd: Conv2d bias + MaxPool2d((p,1)) + PReLU(C) (models.py:187-189) of the products z (planes, H, W),
 *   planes = B C: v (planes, H/p, W) = window maximum of z + bias[c] (first maximum wins; rows beyond (H/p) p are dropped), out = v > 0 ? v : slope[c] v,
 *   amax = row offset of the maximum; backward: dz (planes, H, W) routed (zero elsewhere), part (planes, 2) = {sum of dz
 *   (bias gradient), sum of g v where v <= 0 (slope gradient)} -> mx_reduce_rows over the clips.
 * mx_binmean_head_fwd / _bwd: latent (B, C, W) = mean over bins of x (B, C, H, W), out (B, L, W) = sigmoid(Conv1d(C, L, 1))
 *   (models.py:209-215); backward from d_out (B, L, W) and / or d_latent (B, C, W) (either may be NULL): ds (B, L, W) = the
 *   gradient at the Conv1d output (its weight / bias gradients are an mx_sgemm_f32 / mx_row_sums of it), dx (B, C, H, W).
 * mx_row_sums: out[r] = sum of the n contiguous elements of row r (fp64 accumulate). */
int mx_im2col2d(const float *x, int64_t nb, int64_t Cin, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t dh, int64_t dw,
                int64_t pt, int64_t pl, float *col, void *stream);
int mx_col2im2d(const float *dcol, int64_t nb, int64_t Cin, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t dh, int64_t dw,
                int64_t pt, int64_t pl, float *dx, void *stream);
int mx_rowln_fwd(const float *x, int64_t rows, int64_t n, float eps, float *y, float *stats, void *stream);
int mx_rowln_bwd(const float *dy, const float *y, const float *stats, int64_t rows, int64_t n, float *dx, void *stream);
int mx_row_sums(const float *x, int64_t rows, int64_t n, float *out, void *stream);
int mx_pool_prelu_fwd(const float *z, const float *bias, int64_t planes, int64_t C, int64_t H, int64_t W, int64_t p,
                      const float *slope, float *v, float *out, uint8_t *amax, void *stream);
int mx_pool_prelu_bwd(const float *g, const float *v, const uint8_t *amax, int64_t planes, int64_t C, int64_t H, int64_t W,
                      int64_t p, const float *slope, float *dz, float *part, void *stream);
int mx_binmean_head_fwd(const float *x, int64_t B, int64_t C, int64_t H, int64_t W, const float *wout, const float *bout,
                        int64_t L, float *latent, float *out, void *stream);
int mx_binmean_head_bwd(const float *d_out, const float *d_latent, const float *out, const float *wout, int64_t B, int64_t C,
                        int64_t H, int64_t W, int64_t L, float *ds, float *dx, void *stream);

/* ---- LSTMEffectModel of any size -- mod_extraction/models.py:311-339 with in_ch / out_ch / n_hidden / latent_dim other than
 * the shipped 1 / 1 / 64 / 1 (a param_model, lightning.py:344-347, widens latent_dim).  Only the recurrences are kernels of
 * their own; the input projection, the output layer and every gradient product are mx_sgemm_f32 calls over all steps.
 * mx_lstmg_fwd: zin (B, T, 4 Hn) = W_ih u_t (gate order i, f, g, o); per step gates = act(zin + bias_ih + bias_hh + W_hh h),
 *   c = f c + i g, h = o tanh(c); stash (B, T, 6, Hn) = (i, f, g, o, c, h) of every step; (h1, c1) = the final state.
 * mx_lstmg_bwd: dhfc (B, T, Hn) = d loss / d h_t through the output layer; dgate (B, T, 4 Hn) = d loss / d gate
 *   pre-activations (BPTT inside the chunk; the incoming state is a constant, lightning.py:353,383).
 * mx_lstmg_out_fwd: y (B, Co, T) = tanh(fc (B, T, out_ch) + bias + x (B, in_ch, T)), Co = max(out_ch, in_ch), torch's
 *   broadcast (models.py:337-338).  mx_lstmg_out_bwd: dpre (B, T, out_ch) = dy (1 - y^2) summed over the broadcast channels. */
int mx_lstmg_fwd(const float *zin, const float *bias_ih, const float *bias_hh, const float *w_hh, const float *h0, const float *c0,
                 int64_t B, int64_t T, int64_t Hn, float *stash, float *h1, float *c1, void *stream);
int mx_lstmg_bwd(const float *stash, const float *dhfc, const float *w_hh, const float *c0, int64_t B, int64_t T, int64_t Hn,
                 float *dgate, void *stream);
int mx_lstmg_out_fwd(const float *fc, const float *bias, const float *x, int64_t B, int64_t T, int64_t out_ch, int64_t in_ch,
                     float *y, void *stream);
int mx_lstmg_out_bwd(const float *dy, const float *y, int64_t B, int64_t T, int64_t out_ch, int64_t Co, float *dpre, void *stream);

/* ---- TCN variants outside SpectralTCN / SpectralDSTCN -- mod_extraction/tcn.py:14-103,130-195: explicit padding with the causal /
 * centre crop of the residual branch, the cached streaming convolution, FiLM with or without its BatchNorm1d.  Dense
 * (B, C, T) fp32 tensors of any length; convolutions = mx_im2col2d (one bin row) + mx_sgemm_f32, LayerNorm = mx_rowln_*.
 * mx_chan_stats: stats (C, 2) = {mean, biased variance} of every channel over (clips, frames) (BatchNorm1d training mode).
 * mx_chan_norm_fwd: xhat = (z - norm[c][0]) norm[c][1], norm (C, 2) = {mean, rstd}; _bwd: dz = rstd (g - mean(g) - xhat
 *   mean(g xhat)) with the means over (clips, frames) when train != 0 (batch statistics), else dz = rstd g.
 * mx_film_fwd: a = xhat gb[b][c] + gb[b][C + c], gb (B, 2 C) = the adaptor's output (tcn.py:95-102); _bwd: dxhat = da gain,
 *   dgb = {sum over frames of da xhat, of da}.
 * mx_prelu_res_fwd: y = PReLU(a; slope[c]) (slope NULL: identity) + res (NULL: none) (tcn.py:185-191); _bwd: da = dy PReLU'(a),
 *   part (B C,) = sum over frames of dy a where a <= 0 (slope gradient after mx_reduce_rows over the clips). */
int mx_chan_stats(const float *z, int64_t B, int64_t C, int64_t T, float *stats, void *stream);
int mx_chan_norm_fwd(const float *z, const float *norm, int64_t B, int64_t C, int64_t T, float *xhat, void *stream);
int mx_chan_norm_bwd(const float *g, const float *xhat, const float *norm, int64_t B, int64_t C, int64_t T, int32_t train, float *dz,
                     void *stream);
int mx_film_fwd(const float *xhat, const float *gb, int64_t B, int64_t C, int64_t T, float *a, void *stream);
int mx_film_bwd(const float *da, const float *xhat, const float *gb, int64_t B, int64_t C, int64_t T, float *dxhat, float *dgb,
                void *stream);
int mx_prelu_res_fwd(const float *a, const float *slope, const float *res, int64_t B, int64_t C, int64_t T, float *y, void *stream);
int mx_prelu_res_bwd(const float *dy, const float *a, const float *slope, int64_t B, int64_t C, int64_t T, float *da, float *part,
                     void *stream);

/* ---- effect-model losses -- mod_extraction/losses.py:14-67 (ESR, DC) and nn.L1Loss:
 * part (B,4) = per-clip sums of |y - y_hat|, (y - y_hat)^2, y^2, (y - y_hat). */
int mx_effect_loss_sums(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                        int64_t T, float *part, void *stream);
/* d (w_l1 L1 + w_mse MSE + w_esr ESR + w_dc DC) / d y_hat ('mean' reductions; nn.L1Loss, nn.MSELoss, losses.py:33-38,
 * 61-66) into dy (B rows, stride dy_stride); accumulate != 0 adds onto what dy holds (e.g. the MR-STFT gradient).
 * The backward half of losses.py:142-160 for the effect model (lightning.py:380-382). */
int mx_effect_loss_grad(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                        int64_t T, float w_l1, float w_mse, float w_esr, float w_dc, float eps, int32_t accumulate,
                        float *dy, int64_t dy_stride, void *stream);

/* ---- K11: multi-resolution STFT loss -- mod_extraction/losses.py:155-156 (auraloss==0.4.0
 * MultiResolutionSTFTLoss(reduction="mean"), third-party: restated from its published defaults,
 * parity unpinned): mean over resolutions of [ w_sc * ||Y-X||_F/||Y||_F + w_log * mean|log X - log Y| ],
 * mag = sqrt(clamp(re^2+im^2, eps)).  y_hat, y: B rows of T samples (row strides).
 * fft_sizes, hops: HOST int32 arrays of n_res entries (fft sizes in {512,1024,2048}) -- the only host
 * pointers of this ABI.  windows (n_res, 2048) device: row r = n_fft_r-long analysis window (hann of
 * win_length centred in the frame).  twiddle (2048,2) device = exp(-2 pi i m/2048).
 * terms (2*n_res+1) device: [sc_0, logmag_0, ..., total].  dx: d total / d y_hat rows (stride dx_stride)
 * or NULL.  Workspaces (device): part >= 3*B*max_r ceil(frames_r/8) doubles, coef n_res floats (the scalar alpha_r =
 * w_sc / (n_res ||Y-X||_F ||Y||_F) of each resolution), scratch (needed only when dx != NULL) >= sum_r 2*B*(frames_r*hop_r +
 * runs_r*max(n_fft_r - hop_r, 0)) floats with frames_r = 1 + T/hop_r, runs_r = ceil(frames_r/F_r), F_r = max(32,
 * ceil(n_fft_r/hop_r)) rounded up to even: the two linear components g1_r, g2_r of the time-domain gradient
 * (d total / d y_hat = sum_r alpha_r g1_r + g2_r) as per-run overlap-add sums plus one tail per run; nothing per bin is stored. */
int mx_mrstft_loss(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                   int64_t T, int32_t n_res, const int32_t *fft_sizes, const int32_t *hops,
                   const float *windows, const float *twiddle, float w_sc, float w_log, float eps,
                   double *part, float *coef, float *scratch, float *terms, float *dx, int64_t dx_stride,
                   void *stream);

/* ---- K13: log-mel L1 loss -- mod_extraction/losses.py:105-130 (LogMelLoss: torchaudio MelSpectrogram with centre / reflect
 * padding of n_fft/2, periodic hann, power 2, HTK filter bank, no norm):
 * value = scale * mean |log max(mel(y_hat), eps) - log max(mel(y), eps)| over B x n_mels x frames, frames = 1 + T/hop, and
 * dx (+)= d value / d y_hat (torch's conventions: sgn(0) = 0, the clamp passes the gradient where mel >= eps).
 * y_hat, y: B rows of T samples (row strides); window (n_fft,); twiddle (n_fft, 2) = exp(-2 pi i m / n_fft);
 * fb (n_fft/2+1, n_mels) row-major; band_lo / band_hi (n_mels,) int32 non-zero row range of each band (mx_logmel_fwd's tables).
 * n_fft in {512, 1024, 2048} (else MX_ERR_UNSUPPORTED); any hop > 0; n_mels <= 2048 within the LDS budget (else
 * MX_ERR_UNSUPPORTED); eps > 0; T <= n_fft/2 (the reflect padding needs more samples): MX_ERR_ARG, before any launch.
 * value: one device float (written, never accumulated).  dx (B rows, stride dx_stride) or NULL (value only: no inverse
 * transforms); accumulate != 0 adds the scaled gradient onto what dx holds.  Workspaces (device): part >= B * ceil(frames / 32)
 * doubles (per-workgroup partial sums); scratch (only when dx != NULL) >= B * (frames * hop + runs * max(n_fft - hop, 0))
 * floats with runs = ceil(frames / F), F = max(32, ceil(n_fft / hop)) rounded up to even: the time-domain gradient as
 * per-run overlap-add sums plus one tail per run; nothing per bin is stored.  Deterministic: no float atomics. */
int mx_logmel_l1_loss(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B, int64_t T,
                      const float *window, const float *twiddle, const float *fb, const int32_t *band_lo,
                      const int32_t *band_hi, int64_t n_fft, int64_t hop, int64_t n_mels, float eps, float scale,
                      int32_t accumulate, double *part, float *scratch, float *value, float *dx, int64_t dx_stride,
                      void *stream);

/* ---- K15: FIR pre-emphasis and the ESR taken after it (csrc/pre_emph_loss.hip) -- mod_extraction/wright_code.py:47-73
 * (WrightPreEmph; Conv1d is a cross-correlation) and losses.py:34-38 (ESRLoss) on its outputs.  The linear map F on a row
 * x[0..T), taps (K,) a device pointer, the stages applied one after the other in fp32:
 *   stage 1  f[n] = sum_k taps[k] x[n-(K-1)+k], n = 0..T-1, x[<0] = 0;
 *   stage 2  (low_pass != 0 only, taps [0.85, 1], no padding)  g[n] = 0.85 f[n] + f[n+1], n = 0..T-2;
 * so F x has L = T entries without low_pass and T - 1 with it.  F^T is the exact transpose of the two stages, boundary rows
 * included.  All rows carry a row stride.  NULL pointers, B <= 0, T <= 0, L <= 0 (T == 1 with low_pass), an output stride
 * below the output row length: MX_ERR_ARG; K < 1, K > 16 or T >= 2^30: MX_ERR_UNSUPPORTED; all before any launch.
 *
 * mx_pre_emph: out[b, 0..L) = F(x[b, 0..T)); transpose != 0: out[b, 0..T) = F^T(x[b, 0..L)) (the backward of the former).
 * x_stride must cover the input row (else MX_ERR_ARG); B <= 65535. */
int mx_pre_emph(const float *x, int64_t x_stride, int64_t B, int64_t T, const float *taps, int64_t K, int32_t low_pass,
                int32_t transpose, float *out, int64_t out_stride, void *stream);
/* part (B, 2) = per-clip ( sum (F(y - y_hat))^2, sum (F y)^2 ): fp64 sums in a fixed order, no atomics.  The pre-emphasised
 * ESR is mean_b part[b,0] / (part[b,1] + eps). */
int mx_pre_emph_esr_sums(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B, int64_t T,
                         const float *taps, int64_t K, int32_t low_pass, float *part, void *stream);
/* dy (B rows of T samples, stride dy_stride >= T, also when L = T - 1) = or (accumulate != 0) +=
 *   w * d/d y_hat [ mean_b sum (F(y - y_hat))^2 / (sum (F y)^2 + eps) ] = (2 w / B) F^T F (y_hat - y) / (sum (F y)^2 + eps),
 * and part as mx_pre_emph_esr_sums leaves it: one launch gives value and gradient (one workgroup per clip, a reduction sweep,
 * then the write sweep while the row is cache-resident, as mx_effect_loss_grad). */
int mx_pre_emph_esr_grad(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B, int64_t T,
                         const float *taps, int64_t K, int32_t low_pass, float w, float eps, int32_t accumulate,
                         float *part, float *dy, int64_t dy_stride, void *stream);

/* ---- K12: AdamW -- torch.optim.AdamW (configs/opt/adam_w.yml), flat fp32 buffers of n elements;
 * step = 1-based step index; grad_scale multiplies the gradient first (1/world after a sum
 * all-reduce). */
int mx_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                  int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                  float grad_scale, void *stream);

/* mx_reduce_rows + mx_adamw_step in ONE launch for small parameter sets whose gradient arrives as one row per clip (the
 * LSTM-64's 17 473 parameters, 83 optimizer steps per TBPTT batch: lightning.py:355-384 / configs/opt/adam_w.yml):
 * part (R, n) -> grad (n,) = column sums (fp64, the order of mx_reduce_rows), then the AdamW update of mx_adamw_step on them.
 * Bit-identical to the two calls. */
int mx_reduce_rows_adamw_step(const float *part, int64_t R, float *param, float *grad, float *exp_avg, float *exp_avg_sq,
                              int64_t n, int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                              float grad_scale, void *stream);

/* ---- K12 with gradient clipping (csrc/optim_clip.hip) -- the trainer keys gradient_clip_val / gradient_clip_algorithm of
 * the reference's configs/trained/ files, i.e. torch.nn.utils.clip_grad_norm_ (2-norm) and clip_grad_value_ on the one flat
 * gradient; the clip coefficient is formed and consumed on the device.
 *
 * mx_grad_sumsq: stat[0] = sum of grad[i]^2, i in [0, n), in fp64 (squares exact).  Two launches: workgroup w of G sums the
 * 4096-element chunks w, w + G, ... into part[w] (fixed order inside the workgroup), then one workgroup adds part[0..G) in index
 * order.  No atomics: the same data gives the same bits.  part: at least G doubles, stat: at least 2 doubles (stat[1] is not
 * written here); grad is only read.
 *   G = mx_sumsq_partials(n) = min(ceil(n / 4096), 1024)      (restated as optim.sumsq_partials in the Python package)
 * NULL pointers or n <= 0: MX_ERR_ARG. */
int mx_grad_sumsq(const float *grad, int64_t n, double *part, double *stat, void *stream);

/* mx_adamw_step with the clip applied to the gradient as it is read (grad itself stays un-clipped); all else as mx_adamw_step.
 *   clip_mode 1 (norm):  norm = sqrt(stat[0]) * (double)grad_scale;  coef = min(1.0, (double)clip_val / (norm + 1e-6));
 *                        s = (float)((double)grad_scale * coef);  gi = grad[i] * s.  stat[0] from mx_grad_sumsq on the same
 *                        stream.  coef == 1 gives s == grad_scale and the bits of mx_adamw_step.
 *   clip_mode 2 (value): t = grad[i] * grad_scale;  gi = t > c ? c : (t < -c ? -c : t), c = clip_val (a NaN stays a NaN, as
 *                        under torch.clamp); stat[0] is not read and s = grad_scale.
 * stat[1] = (double)s is written by one thread.  NULL pointers, step <= 0, n <= 0, a mode outside {1, 2} or a clip_val that is
 * not finite and positive: MX_ERR_ARG. */
int mx_adamw_step_clip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step, float lr,
                       float beta1, float beta2, float eps, float weight_decay, float grad_scale, int32_t clip_mode,
                       float clip_val, double *stat, void *stream);

/* ---- K16: learned effect parameters of the audio-loss step (csrc/fx_params.hip) -- no counterpart in the reference, whose
 * steps read every effect parameter from the batch.  P <= 16 shared scalars raw (P,) fp32, one per learned (kind, name) pair:
 *   s = sigmoid(raw_gain * raw[e]);  value = lo + (hi - lo) s,  or with the log flag  exp(log lo + (log hi - log lo) s),
 * in fp64.  The table: tab_f (2, P) fp64 = the rows lo, hi; tab_i (3, P) int32 = the rows log flag, slot, kind.  Slots, in
 * this order: lfo_scale 0, min_delay 1, feedback 2, depth 3, mix 4, centre_frequency_hz 5.  Kinds: flanger 0, chorus 1,
 * phaser 2, tremolo 3, dry 4; row_kind (B,) int32 gives every row's.  max_lfo_delay / max_min_delay (B,) fp32: the per-row
 * sample counts the lfo_scale / min_delay slots are scaled with.  NULL table / raw / row_kind, P <= 0, B <= 0: MX_ERR_ARG;
 * P > 16: MX_ERR_UNSUPPORTED; all before any launch.
 *
 * mx_fx_params_expand: every entry writes (float)value into the rows of its kind of its slot's (B,) fp32 vector (one thread
 * per row); lfo_scale / min_delay are then multiplied with the row's sample count in fp32, one_minus_mix = 1 - mix in fp32
 * wherever mix is written.  Rows and slots without an entry are not written; a NULL output skips its slot (an lfo_scale /
 * min_delay output without its count vector: MX_ERR_ARG).  values (P,) fp32, optional: the mapped values. */
int mx_fx_params_expand(const float *raw, const double *tab_f, const int32_t *tab_i, int64_t P, double raw_gain,
                        const int32_t *row_kind, const float *max_lfo_delay, const float *max_min_delay, int64_t B,
                        float *lfo_scale, float *min_delay, float *feedback, float *depth, float *mix, float *one_minus_mix,
                        float *centre_frequency_hz, float *values, void *stream);
/* d_raw (P,) fp32 = scale * d loss / d raw from grads (6, B) fp64, row s = the per-clip d loss / d (slot s) the effect
 * adjoints write: per entry (one workgroup each) the rows of its kind, times the sample count where the slot has one, summed
 * in fp64 in a fixed order, times d value / d raw and scale in fp64, rounded once.  Rows of other kinds are not read.  No
 * atomics, no workspace: deterministic.  Both count vectors are required. */
int mx_fx_params_grad(const double *grads, const float *raw, const double *tab_f, const int32_t *tab_i, int64_t P,
                      double raw_gain, const int32_t *row_kind, const float *max_lfo_delay, const float *max_min_delay,
                      int64_t B, double scale, float *d_raw, void *stream);

/* ---- K17: effect parameters per clip, from a linear head on the extractor's latent (csrc/fx_head.hip) -- no counterpart in
 * the reference.  The table, the slots, the kinds, raw_gain, row_kind and the sample counts are those of K16 (above);
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

/* ---- K22: one LFO track along a whole recording from the LFOs of overlapping windows (csrc/lfo_stitch.hip) -- no
 * counterpart in the reference.
 * windows (W, n_f) fp32, dense: row w is the LFO the extractor gave for the N samples that start at sample starts[w] of a
 * recording of L samples.  Its n_f points sit at the sample positions
 *
 *   starts[w] + i (N - 1) / (n_f - 1),   i = 0 .. n_f - 1
 *
 * (the align_corners rule by which the effect kernels spread a low-rate LFO over a clip).  Track point j sits at
 *
 *   p_j = j (L - 1) / (n_t - 1),         j = 0 .. n_t - 1
 *
 * and over the windows with starts[w] <= p_j <= starts[w] + N - 1, in ascending w,
 *
 *   track[j] = sum_w a_w v_w / sum_w a_w,     cover[j] = the number of those windows
 *   v_w = the linear interpolation of row w at p_j:  t = (p_j - starts[w]) (n_f - 1) / (N - 1),  i0 = min(floor(t), n_f - 2),
 *         f = t - i0,  v_w = (1 - f) x[i0] + f x[i0 + 1]
 *   a_w = sin^2(pi u) + 1e-3,  u = (p_j - starts[w] + 0.5) / N
 *
 * The taper is there because a window's edge frames are the extractor's least reliable; the floor keeps a point that only
 * window edges cover (the recording's two ends) defined.  Positions, weights and both sums are fp64; there is one rounding
 * to fp32.  A point that no window covers gets cover 0 and track 0.  One thread per track point, no atomics, no workspace:
 * the same arguments give the same bits.  starts: (W,) int64 on the device, ascending (not checked: they live on the
 * device; an unsorted list gives a defined, but other, window range).
 * Before any launch: a NULL pointer, W < 1, n_f < 2, N < 2, L < N, n_t < 2, an output that overlaps an input or the other
 * output: MX_ERR_ARG.  W > MX_STITCH_MAX_WINDOWS, L > 2^31, n_f > 2^22 or n_t > 2^22: MX_ERR_UNSUPPORTED (so j (L - 1) is
 * exact in fp64, p_j is ONE correctly rounded division, and its comparisons with the integers starts[w] and
 * starts[w] + N - 1 are those of the exact rational). */
#define MX_STITCH_MAX_WINDOWS (1 << 20)

int mx_lfo_stitch(const float *windows, const int64_t *starts, int64_t W, int64_t n_f, int64_t N, int64_t L, int64_t n_t,
                  float *track, int32_t *cover, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_HIP_H */
