// fx_head.hip -- K17: effect parameters PER CLIP, predicted by one linear layer on the mean-pooled latent of the extractor
// (no counterpart in the reference, whose steps read every effect parameter from the batch).  The table, the slots, the kinds
// and the map are those of fx_params.hip (fx_params_common.h); what differs is where raw comes from:
//     pooled[b, c] = mean_w latent[b, c, w]                       fp64 sum in a fixed order, rounded to fp32 once
//     raw[b, e]    = bias[e] + sum_c weight[e, c] pooled[b, c]    fp64 from the fp32 pooled, fixed order, rounded once
//     value[b, e]  = fxp_value((double)raw[b, e], ...)            rounded once
// Because the value is taken from the fp32 raw, a head with weight == 0 writes the bits mx_fx_params_expand writes for
// raw = bias.
//
// mx_fx_head_fwd  one 256-thread workgroup per clip.  The four waves take the channels in turn, the lanes stride along w
//     (consecutive lanes read consecutive floats; a row of W floats is in general not 16-byte aligned, so the loads stay
//     scalar), the lanes are combined by the fp64 butterfly.  pooled stays in LDS for the linear layer: the waves take the
//     entries in turn, the lanes stride along c.  Lane 0 maps the value and, on a row of the entry's kind, writes it into the
//     row of its slot's vector by the rule of mx_fx_params_expand.  No atomics, no workspace beyond the outputs.
// mx_fx_head_bwd  two independent launches.  With d_raw[b, e] = scale * grads[slot_e, b] * (the row's sample count where the
//     slot has one) * d value / d raw at raw[b, e] on the rows of the entry's kind (fp64; elsewhere 0, and grads is not read):
//     rows kernel, one workgroup per clip: d_raw_rows[b, :], then d_latent[b, c, :] = (1 / W) sum_e d_raw[b, e] weight[e, c],
//         one fp32 per channel in LDS, stored over the clip's C W contiguous floats: float4 where the address is 16-byte
//         aligned, a scalar head and tail around it.  Every element is written; a row without an entry gets exact zeros (the
//         sum has no term then).
//     sums kernel, one wave per (entry, column): d_weight[e, c] = sum_b d_raw[b, e] pooled[b, c] and (column C) d_bias[e] =
//         sum_b d_raw[b, e], the lanes striding along b in row order, then the butterfly; d_raw is recomputed from grads (a few
//         fp64 operations), so nothing passes between the launches.
//     Every output is one fp32 rounding of an fp64 sum in a fixed order: the same inputs give the same bits.
// Both entries are latency- and streaming-bound: the latent is read once, d_latent is written once.
#include "fx_params_common.h"
#include "rows_common.h"

#define FXH_MAX_C 1024
#define FXH_WAVES (FXP_THREADS / MX_WAVE)

__global__ __launch_bounds__(FXP_THREADS) void fx_head_fwd_kernel(
    const float *__restrict__ latent, int C, int W, const float *__restrict__ weight, const float *__restrict__ bias,
    const double *__restrict__ tab_f, const int *__restrict__ tab_i, int P, double gain, const int *__restrict__ row_kind,
    const float *__restrict__ max_lfo_delay, const float *__restrict__ max_min_delay, FxpOut out, float *__restrict__ pooled,
    float *__restrict__ raw_rows, float *__restrict__ values)
{
    __shared__ float pool_s[FXH_MAX_C];
    const size_t b = blockIdx.x;
    const int lane = (int)(threadIdx.x & (MX_WAVE - 1)), wave = (int)(threadIdx.x / MX_WAVE);
    const float *lb = latent + b * (size_t)C * (size_t)W;
    for (int c = wave; c < C; c += FXH_WAVES) {                 // wave-uniform: every lane reaches the butterfly
        const float *row = lb + (size_t)c * (size_t)W;
        double s = 0.0;
        for (int w = lane; w < W; w += MX_WAVE) s += (double)row[w];
        s = wave_sum_f64(s);
        if (lane == 0) {
            const float p = (float)(s / (double)W);
            pool_s[c] = p;
            pooled[b * (size_t)C + c] = p;
        }
    }
    __syncthreads();
    const int kind = row_kind[b];
    for (int e = wave; e < P; e += FXH_WAVES) {
        const float *we = weight + (size_t)e * (size_t)C;
        double s = 0.0;
        for (int c = lane; c < C; c += MX_WAVE) s += (double)we[c] * (double)pool_s[c];
        s = wave_sum_f64(s);
        if (lane != 0) continue;
        const float r = (float)((double)bias[e] + s);
        raw_rows[b * (size_t)P + e] = r;
        float v = (float)fxp_value((double)r, gain, tab_f[e], tab_f[P + e], tab_i[e], nullptr);
        if (values) values[b * (size_t)P + e] = v;
        const int slot = tab_i[P + e];
        if (tab_i[2 * P + e] != kind || slot < 0 || slot >= FXP_SLOTS || !out.v[slot]) continue;
        if (slot == FXP_LFO_SCALE) v = __fmul_rn(v, max_lfo_delay[b]);
        if (slot == FXP_MIN_DELAY) v = __fmul_rn(v, max_min_delay[b]);
        out.v[slot][b] = v;
        if (slot == FXP_MIX && out.one_minus_mix) out.one_minus_mix[b] = __fsub_rn(1.0f, v);
    }
}

// d_raw[b, e] in fp64; *active = 0 (and 0.0, with grads not read) where row b is not of the entry's kind
__device__ __forceinline__ double fxh_d_raw(const double *__restrict__ grads, const float *__restrict__ raw_rows,
                                            const double *__restrict__ tab_f, const int *__restrict__ tab_i, int P, double gain,
                                            const int *__restrict__ row_kind, const float *__restrict__ max_lfo_delay,
                                            const float *__restrict__ max_min_delay, size_t B, double scale, size_t b, int e,
                                            int *active)
{
    const int slot = tab_i[P + e];
    *active = (slot >= 0 && slot < FXP_SLOTS && row_kind[b] == tab_i[2 * P + e]) ? 1 : 0;
    if (!*active) return 0.0;
    double t = grads[(size_t)slot * B + b];
    if (slot == FXP_LFO_SCALE) t *= (double)max_lfo_delay[b];
    if (slot == FXP_MIN_DELAY) t *= (double)max_min_delay[b];
    double dv;
    fxp_value((double)raw_rows[b * (size_t)P + e], gain, tab_f[e], tab_f[P + e], tab_i[e], &dv);
    return t * dv * scale;
}

__global__ __launch_bounds__(FXP_THREADS) void fx_head_bwd_rows_kernel(
    const double *__restrict__ grads, const float *__restrict__ raw_rows, const float *__restrict__ weight,
    const double *__restrict__ tab_f, const int *__restrict__ tab_i, int P, double gain, const int *__restrict__ row_kind,
    const float *__restrict__ max_lfo_delay, const float *__restrict__ max_min_delay, size_t B, int C, int W, double scale,
    float *__restrict__ d_raw_rows, float *__restrict__ d_latent)
{
    __shared__ double dr[FXP_MAX_ENTRIES];
    __shared__ int act[FXP_MAX_ENTRIES];
    __shared__ float cv[FXH_MAX_C];
    const size_t b = blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (tid < P) {
        int a;
        const double d = fxh_d_raw(grads, raw_rows, tab_f, tab_i, P, gain, row_kind, max_lfo_delay, max_min_delay, B, scale, b,
                                   tid, &a);
        dr[tid] = d;
        act[tid] = a;
        if (d_raw_rows) d_raw_rows[b * (size_t)P + tid] = (float)d;
    }
    if (!d_latent) return;                                      // uniform over the grid
    __syncthreads();
    for (int c = tid; c < C; c += FXP_THREADS) {
        double s = 0.0;
        for (int e = 0; e < P; ++e)
            if (act[e]) s += dr[e] * (double)weight[(size_t)e * (size_t)C + c];
        cv[c] = (float)(s / (double)W);
    }
    __syncthreads();
    // the clip's C W contiguous floats: element i belongs to channel i / W
    float *ob = d_latent + b * (size_t)C * (size_t)W;
    const int n = C * W;
    int head = rows_head(ob);
    if (head > n) head = n;
    const int nv = (n - head) >> 2;
    for (int i = tid; i < head; i += FXP_THREADS) ob[i] = cv[i / W];
    for (int q = tid; q < nv; q += FXP_THREADS) {
        const int i = head + 4 * q;
        int c = i / W, r = i - c * W;
        float4 o;
        o.x = cv[c]; if (++r == W) { r = 0; ++c; }
        o.y = cv[c]; if (++r == W) { r = 0; ++c; }
        o.z = cv[c]; if (++r == W) { r = 0; ++c; }
        o.w = cv[c];
        *(float4 *)(ob + i) = o;
    }
    for (int i = head + 4 * nv + tid; i < n; i += FXP_THREADS) ob[i] = cv[i / W];
}

__global__ __launch_bounds__(FXP_THREADS) void fx_head_bwd_sums_kernel(
    const double *__restrict__ grads, const float *__restrict__ raw_rows, const float *__restrict__ pooled,
    const double *__restrict__ tab_f, const int *__restrict__ tab_i, int P, double gain, const int *__restrict__ row_kind,
    const float *__restrict__ max_lfo_delay, const float *__restrict__ max_min_delay, size_t B, int C, double scale,
    float *__restrict__ d_bias, float *__restrict__ d_weight)
{
    const int e = (int)blockIdx.x;
    const int lane = (int)(threadIdx.x & (MX_WAVE - 1));
    const int j = (int)blockIdx.y * FXH_WAVES + (int)(threadIdx.x / MX_WAVE);     // column: a channel, or C = the bias
    if (j > C || (j == C ? !d_bias : !d_weight)) return;                          // wave-uniform; no barrier below
    double s = 0.0;
    for (size_t b = (size_t)lane; b < B; b += MX_WAVE) {
        int a;
        const double d = fxh_d_raw(grads, raw_rows, tab_f, tab_i, P, gain, row_kind, max_lfo_delay, max_min_delay, B, scale, b,
                                   e, &a);
        if (a) s += j < C ? d * (double)pooled[b * (size_t)C + j] : d;
    }
    s = wave_sum_f64(s);
    if (lane != 0) return;
    if (j < C) d_weight[(size_t)e * (size_t)C + j] = (float)s;
    else d_bias[e] = (float)s;
}

// C ABI ---------------------------------------------------------------------------------------
// latent (B, C, W) fp32 dense; weight (P, C), bias (P,) fp32; the table, raw_gain, row_kind and the sample counts as given to
// mx_fx_params_expand; the seven (B,) fp32 constant vectors, each optional (NULL: entries of that slot are skipped).  Outputs:
// pooled (B, C) and raw_rows (B, P) fp32 (required: the backward reads them), values (B, P) fp32 (optional).
MX_EXPORT int mx_fx_head_fwd(const float *latent, int64_t B, int64_t C, int64_t W, const float *weight, const float *bias,
                             const double *tab_f, const int32_t *tab_i, int64_t P, double raw_gain, const int32_t *row_kind,
                             const float *max_lfo_delay, const float *max_min_delay, float *lfo_scale, float *min_delay,
                             float *feedback, float *depth, float *mix, float *one_minus_mix, float *centre_frequency_hz,
                             float *pooled, float *raw_rows, float *values, void *stream)
{
    if (!latent || !weight || !bias || !tab_f || !tab_i || !row_kind || !pooled || !raw_rows || P <= 0 || B <= 0 || C <= 0 ||
        W <= 0)
        return MX_ERR_ARG;
    if ((lfo_scale && !max_lfo_delay) || (min_delay && !max_min_delay)) return MX_ERR_ARG;
    if (P > FXP_MAX_ENTRIES || C > FXH_MAX_C || B >= (1ll << 30) || W >= (1ll << 30) || C * W >= (1ll << 31))
        return MX_ERR_UNSUPPORTED;
    FxpOut out;
    out.v[FXP_LFO_SCALE] = lfo_scale; out.v[FXP_MIN_DELAY] = min_delay; out.v[FXP_FEEDBACK] = feedback;
    out.v[FXP_DEPTH] = depth; out.v[FXP_MIX] = mix; out.v[FXP_CENTRE] = centre_frequency_hz;
    out.one_minus_mix = one_minus_mix;
    hipLaunchKernelGGL(fx_head_fwd_kernel, dim3((unsigned)B), dim3(FXP_THREADS), 0, (hipStream_t)stream, latent, (int)C, (int)W,
                       weight, bias, tab_f, tab_i, (int)P, raw_gain, row_kind, max_lfo_delay, max_min_delay, out, pooled,
                       raw_rows, values);
    return mx_launch_status();
}

// grads (6, B) fp64 as given to mx_fx_params_grad (only the rows of an entry's kind of an entry's slot are read); raw_rows
// (B, P) and pooled (B, C) as mx_fx_head_fwd wrote them; weight (P, C); both count vectors are required.  Outputs, each fp32
// and optional: d_raw_rows (B, P), d_bias (P,), d_weight (P, C), d_latent (B, C, W) dense (every element written).
MX_EXPORT int mx_fx_head_bwd(const double *grads, const float *raw_rows, const float *pooled, const float *weight,
                             const double *tab_f, const int32_t *tab_i, int64_t P, double raw_gain, const int32_t *row_kind,
                             const float *max_lfo_delay, const float *max_min_delay, int64_t B, int64_t C, int64_t W,
                             double scale, float *d_raw_rows, float *d_bias, float *d_weight, float *d_latent, void *stream)
{
    if (!grads || !raw_rows || !pooled || !weight || !tab_f || !tab_i || !row_kind || !max_lfo_delay || !max_min_delay ||
        P <= 0 || B <= 0 || C <= 0 || W <= 0)
        return MX_ERR_ARG;
    if (P > FXP_MAX_ENTRIES || C > FXH_MAX_C || B >= (1ll << 30) || W >= (1ll << 30) || C * W >= (1ll << 31))
        return MX_ERR_UNSUPPORTED;
    if (d_raw_rows || d_latent) {
        hipLaunchKernelGGL(fx_head_bwd_rows_kernel, dim3((unsigned)B), dim3(FXP_THREADS), 0, (hipStream_t)stream, grads,
                           raw_rows, weight, tab_f, tab_i, (int)P, raw_gain, row_kind, max_lfo_delay, max_min_delay, (size_t)B,
                           (int)C, (int)W, scale, d_raw_rows, d_latent);
        const int st = mx_launch_status();
        if (st != MX_OK) return st;
    }
    if (d_bias || d_weight) {
        hipLaunchKernelGGL(fx_head_bwd_sums_kernel, dim3((unsigned)P, (unsigned)((C + 1 + FXH_WAVES - 1) / FXH_WAVES)),
                           dim3(FXP_THREADS), 0, (hipStream_t)stream, grads, raw_rows, pooled, tab_f, tab_i, (int)P, raw_gain,
                           row_kind, max_lfo_delay, max_min_delay, (size_t)B, (int)C, scale, d_bias, d_weight);
    }
    return mx_launch_status();
}
