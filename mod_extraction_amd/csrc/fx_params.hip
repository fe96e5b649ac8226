// fx_params.hip -- K16: the effect parameters the audio-loss step LEARNS (no counterpart in the reference, whose steps read
// every effect parameter from the batch).  P <= 16 shared scalars raw[e], one per learned (kind, name) pair, each mapped onto
// its range
//     s = sigmoid(raw_gain * raw[e]),   value = lo + (hi - lo) s            (lin)
//                                       value = exp(log lo + (log hi - log lo) s)   (log)
// in fp64 and rounded to fp32 once.  The table: tab_f (2, P) fp64 = the rows lo, hi; tab_i (3, P) int32 = the rows log flag,
// slot, kind.  Slots are the per-row constants of the effect launches (FXP_* below), kinds the step's row kinds (flanger 0,
// chorus 1, phaser 2, tremolo 3, dry 4).
//
// mx_fx_params_expand  one thread per row: every entry of the row's kind writes its value into the row of its slot's (B,)
//     vector.  lfo_scale / min_delay then meet the row's fp32 sample count in fp32 (__fmul_rn), one_minus_mix is 1 - mix in
//     fp32: the rule of a tensor parameter in fx.derive_clip_constants.  Rows and slots without an entry are not written.
//     Thread e < P also writes values[e], the mapped value as fp32.
// mx_fx_params_grad    one 256-thread workgroup per entry: the rows of the entry's kind of the slot's row of the (6, B) fp64
//     gradient buffer, each times its sample count where the slot has one, summed in fp64 (per thread in row order, lanes by
//     butterfly, the four waves in order), times d value / d raw and the scale in fp64, rounded once.  No atomics, no
//     workspace: the same inputs give the same bits.  Rows of other kinds are never read (they may be uninitialised).
// Both are launch-latency kernels: a few hundred bytes of traffic each.
#include "fx_params_common.h"

__global__ __launch_bounds__(FXP_THREADS) void fx_params_expand_kernel(
    const float *__restrict__ raw, const double *__restrict__ tab_f, const int *__restrict__ tab_i, int P, double gain,
    const int *__restrict__ row_kind, const float *__restrict__ max_lfo_delay, const float *__restrict__ max_min_delay, int B,
    FxpOut out, float *__restrict__ values)
{
    const int i = (int)(blockIdx.x * FXP_THREADS + threadIdx.x);
    if (i < P && values)
        values[i] = (float)fxp_value((double)raw[i], gain, tab_f[i], tab_f[P + i], tab_i[i], nullptr);
    if (i >= B) return;
    const int kind = row_kind[i];
    for (int e = 0; e < P; ++e) {
        if (tab_i[2 * P + e] != kind) continue;
        const int slot = tab_i[P + e];
        if (slot < 0 || slot >= FXP_SLOTS || !out.v[slot]) continue;
        float v = (float)fxp_value((double)raw[e], gain, tab_f[e], tab_f[P + e], tab_i[e], nullptr);
        if (slot == FXP_LFO_SCALE) v = __fmul_rn(v, max_lfo_delay[i]);
        if (slot == FXP_MIN_DELAY) v = __fmul_rn(v, max_min_delay[i]);
        out.v[slot][i] = v;
        if (slot == FXP_MIX && out.one_minus_mix) out.one_minus_mix[i] = __fsub_rn(1.0f, v);
    }
}

__global__ __launch_bounds__(FXP_THREADS) void fx_params_grad_kernel(
    const double *__restrict__ grads, const float *__restrict__ raw, const double *__restrict__ tab_f,
    const int *__restrict__ tab_i, int P, double gain, const int *__restrict__ row_kind,
    const float *__restrict__ max_lfo_delay, const float *__restrict__ max_min_delay, int B, double scale,
    float *__restrict__ d_raw)
{
    __shared__ double red[4];
    const int e = (int)blockIdx.x;
    const int slot = tab_i[P + e], kind = tab_i[2 * P + e];
    double s = 0.0;
    if (slot >= 0 && slot < FXP_SLOTS) {
        const double *g = grads + (size_t)slot * B;
        for (int b = (int)threadIdx.x; b < B; b += FXP_THREADS) {
            if (row_kind[b] != kind) continue;
            double t = g[b];
            if (slot == FXP_LFO_SCALE) t *= (double)max_lfo_delay[b];
            if (slot == FXP_MIN_DELAY) t *= (double)max_min_delay[b];
            s += t;
        }
    }
    const double total = block256_sum_f64(s, red);
    if (threadIdx.x == 0) {
        double dv;
        fxp_value((double)raw[e], gain, tab_f[e], tab_f[P + e], tab_i[e], &dv);
        d_raw[e] = (float)(total * dv * scale);
    }
}

// C ABI ---------------------------------------------------------------------------------------
// raw (P,) fp32; tab_f (2, P) fp64, tab_i (3, P) int32 (see the head of this file); row_kind (B,) int32; max_lfo_delay,
// max_min_delay (B,) fp32 sample counts (needed only with an lfo_scale / min_delay entry, else they may be NULL).  Outputs,
// each (B,) fp32 and optional (NULL: entries of that slot are skipped): lfo_scale, min_delay, feedback, depth, mix,
// one_minus_mix, centre_frequency_hz; values (P,) fp32, optional.
MX_EXPORT int mx_fx_params_expand(const float *raw, const double *tab_f, const int32_t *tab_i, int64_t P, double raw_gain,
                                  const int32_t *row_kind, const float *max_lfo_delay, const float *max_min_delay, int64_t B,
                                  float *lfo_scale, float *min_delay, float *feedback, float *depth, float *mix,
                                  float *one_minus_mix, float *centre_frequency_hz, float *values, void *stream)
{
    if (!raw || !tab_f || !tab_i || !row_kind || P <= 0 || B <= 0) return MX_ERR_ARG;
    if ((lfo_scale && !max_lfo_delay) || (min_delay && !max_min_delay)) return MX_ERR_ARG;
    if (P > FXP_MAX_ENTRIES || B >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    FxpOut out;
    out.v[FXP_LFO_SCALE] = lfo_scale; out.v[FXP_MIN_DELAY] = min_delay; out.v[FXP_FEEDBACK] = feedback;
    out.v[FXP_DEPTH] = depth; out.v[FXP_MIX] = mix; out.v[FXP_CENTRE] = centre_frequency_hz;
    out.one_minus_mix = one_minus_mix;
    const int64_t n = B > P ? B : P;
    hipLaunchKernelGGL(fx_params_expand_kernel, dim3((unsigned)((n + FXP_THREADS - 1) / FXP_THREADS)), dim3(FXP_THREADS), 0,
                       (hipStream_t)stream, raw, tab_f, tab_i, (int)P, raw_gain, row_kind, max_lfo_delay, max_min_delay, (int)B,
                       out, values);
    return mx_launch_status();
}

// grads (6, B) fp64, row s = d loss / d (slot s) per clip, in the slot order lfo_scale, min_delay, feedback, depth, mix,
// centre_frequency_hz (only the rows of an entry's kind of an entry's slot are read); the table, raw, row_kind and the sample
// counts as given to mx_fx_params_expand (both count vectors are required here).  d_raw (P,) fp32 = scale * d loss / d raw.
MX_EXPORT int mx_fx_params_grad(const double *grads, const float *raw, const double *tab_f, const int32_t *tab_i, int64_t P,
                                double raw_gain, const int32_t *row_kind, const float *max_lfo_delay,
                                const float *max_min_delay, int64_t B, double scale, float *d_raw, void *stream)
{
    if (!grads || !raw || !tab_f || !tab_i || !row_kind || !max_lfo_delay || !max_min_delay || !d_raw || P <= 0 || B <= 0)
        return MX_ERR_ARG;
    if (P > FXP_MAX_ENTRIES || B >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(fx_params_grad_kernel, dim3((unsigned)P), dim3(FXP_THREADS), 0, (hipStream_t)stream, grads, raw, tab_f,
                       tab_i, (int)P, raw_gain, row_kind, max_lfo_delay, max_min_delay, (int)B, scale, d_raw);
    return mx_launch_status();
}
