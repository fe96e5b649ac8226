// phaser_bwd.hip -- K3 adjoint: gradient of the phaser (phaser.hip; oracle_ref.c:orc_phaser) with respect to every
// processed source sample, the LFO and the per-clip depth, centre frequency, feedback and mix, from what
// mx_phaser_fwd_stash left (phaser_common.h).
//
// Per sample n, G the coefficient of its 4-sample group, z = (s0..s5, last) the state BEFORE the sample:
//     out_0 = x - last;   stage k: d_k = out_k - s_k, v_k = G d_k, y_k = v_k + s_k, s_k' = v_k + y_k, out_(k+1) = 2 y_k - out_k
//     last' = fb out_6;   m = mix out_6 + (1 - mix) x;   y = clip(m, -1, 1)
// Adjoint, l_k that of s_k', lam that of last', g_m = dy where -1 <= m <= 1 (aten's clamp rule), sample by sample BACKWARDS:
//     g_out = mix g_m + fb lam;   k = 5..0:  g_y = 2 g_out + l_k, g_v = l_k + g_y, l_k <- g_y - G g_v, g_out <- G g_v - g_out,
//                                           dG += g_v d_k
//     dx = (1 - mix) g_m + g_out;  lam <- -g_out;   d mix += g_m (out_6 - x);   d fb += lam(before) out_6
// and per group  dlfo = dG (1 - G)^2 (pi / sr)(1 + g^2) fc ln10 (log_max - log_min) where 0 <= pre <= 1, else 0 (g = G / (1 - G)):
//     dmod = -dlfo depth (osc = 1 - 2 mod),  d depth += dlfo osc / 2,  d centre += dlfo / (centre ln10 (log_max - log_min)).
//
// The adjoint of a linear time-varying system is one again, so the forward's scan shape runs backwards -- one workgroup per
// clip, one chunk per lane -- and the adjoint's chunk map is the TRANSPOSE of the forward's M, which the stash holds: no
// unit-state runs here.
//   A'  every lane runs the adjoint over its chunk backwards from lam_end = 0 with the masked dy:  lam_start = M^T lam_end + w
//       gives w (the lam recursion needs G and g_m only, no forward value);
//   B'  seven lanes of wave 0 chain the 512 maps from the last chunk to the first: lam_end of every chunk;
//   C'  every lane walks its chunk backwards again from its true lam_end in sub-blocks of PS_SUB groups (8 samples): the
//       forward of the sub-block is recomputed in registers from the stashed state at its start (d_k and out_6 of 8
//       samples: 56 registers), then the adjoint runs over it, writes dx, turns each group's dG into dmod and the depth /
//       centre terms, and accumulates d fb / d mix.  (16-sample sub-blocks need 112 registers for the forward values and
//       spill: 256 VGPRs + 28 B of scratch; 8 samples: 185 VGPRs, no scratch.)
// The four per-clip sums are fp64: per lane, then a butterfly, then the waves in order.  No atomics: two runs give the same
// bits.  Why recompute instead of stashing the stage states of every sample: that stash is 28 B per sample written and read
// with a lane stride of one chunk (64 cache lines per instruction) on top of the forward's 8 B per sample, the
// recomputation is ONE more cascade run per sample where the forward does nine, and the checkpoints cost 4 B per sample
// in 32-byte pieces.
#include "phaser_common.h"

#define PB_S (4 * PS_SUB)                                        // samples per sub-block

// one sample of the adjoint; L = (l_0..l_5, lam); returns g_out after stage 0.  D (the forward's d_k) non-null: dG accumulates.
template <bool WITH_DG>
__device__ __forceinline__ float pb_adj_step(float (&L)[7], float G, float gm, float fb, float wet_g, const float *D, float &dG)
{
    float g_out = __builtin_fmaf(wet_g, gm, fb * L[6]);
#pragma unroll
    for (int k = 5; k >= 0; --k) {
        const float gy = __builtin_fmaf(2.0f, g_out, L[k]);
        const float gv = L[k] + gy;
        const float t = G * gv;
        if (WITH_DG) dG = __builtin_fmaf(gv, D[k], dG);
        L[k] = gy - t;
        g_out = t - g_out;
    }
    L[6] = -g_out;
    return g_out;
}

__global__ __launch_bounds__(PS_P) void phaser_bwd_kernel(
    const float *__restrict__ dy, long long dy_stride, const float *__restrict__ x, long long x_stride, int x_width,
    const float *__restrict__ stash, long long stash_stride, int sg, const float *__restrict__ depth,
    const float *__restrict__ centre, const float *__restrict__ feedback, const float *__restrict__ mix,
    const int *__restrict__ lead_arr, const int *__restrict__ rows, int N, double sr, float *__restrict__ dx,
    long long dx_stride, float *__restrict__ dmod, long long dmod_stride, int n_mod, double *__restrict__ d_depth,
    double *__restrict__ d_centre, double *__restrict__ d_fb, double *__restrict__ d_mix)
{
    extern __shared__ __attribute__((aligned(16))) float pb_lds[];
    __shared__ double red[4][PS_WAVES];
    float *mv = pb_lds, *le = pb_lds + PS_P * PS_MV;
    const int p = threadIdx.x, lane = p & 63;
    const int b = rows ? rows[blockIdx.x] : (int)blockIdx.x;
    const int lead = lead_arr ? lead_arr[b] : 0;
    const int total = lead + N;
    const int n_groups = (total + 3) >> 2;
    if (total > x_width || n_groups > sg) return;                // the forward left this clip alone (whole workgroup)
    const float *xb = x + (size_t)b * x_stride;
    const float *dyb = dy + (size_t)b * dy_stride;
    float *dxb = dx ? dx + (size_t)b * dx_stride : nullptr;
    float *dmb = dmod ? dmod + (size_t)b * dmod_stride : nullptr;
    const PsStash<const float> st = {stash + (size_t)b * stash_stride, sg};

    const PsClip k = ps_clip(sr, 0.0f, depth[b], centre[b], feedback[b], mix[b]);   // (no rate: the phase is not needed)
    const float fb = k.fb, wet_g = k.wet_g;
    const int gpc = (n_groups + PS_P - 1) / PS_P;                // the forward's chunking
    const int g0 = min(p * gpc, n_groups), g1 = min(g0 + gpc, n_groups);

    // the forward's chunk maps -> LDS (M only: slots 49..55 of a chunk take w below)
    for (int i = p; i < PS_P * PS_MV; i += PS_P)
        if (i % PS_MV < 49) mv[i] = st.maps()[i];

    // the masked dy of the four samples of group g
    auto load_gm = [&](int g, float (&gm)[4]) {
        const int pass = st.pass()[g];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 4 * g + j;
            gm[j] = (n >= lead && n < total && ((pass >> j) & 1)) ? dyb[n - lead] : 0.0f;
        }
    };

    // ---- A': w of the chunk
    {
        float L[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, unused = 0.0f;
        for (int g = g1 - 1; g >= g0; --g) {
            const float G = st.G()[g];
            float gm[4];
            load_gm(g, gm);
#pragma unroll
            for (int j = 3; j >= 0; --j) (void)pb_adj_step<false>(L, G, gm[j], fb, wet_g, nullptr, unused);
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) mv[p * PS_MV + 49 + c] = L[c];
    }
    __syncthreads();

    // ---- B': chain the maps backwards (wave 0; lane c < 7 owns component c: (M^T lam)_c = sum_r M[r][c] lam_r)
    if (p < 64) {
        const int c = lane < 7 ? lane : 0;
        float lam[7], mine = 0.0f;
#pragma unroll
        for (int r = 0; r < 7; ++r) lam[r] = 0.0f;
        for (int q = PS_P - 1; q >= 0; --q) {
            if (lane < 7) le[q * 8 + lane] = mine;
            const float *m = mv + q * PS_MV;
            float acc = m[49 + c];
#pragma unroll
            for (int r = 0; r < 7; ++r) acc = __builtin_fmaf(m[c * 7 + r], lam[r], acc);
            mine = acc;
#pragma unroll
            for (int r = 0; r < 7; ++r) lam[r] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), r));
        }
    }
    __syncthreads();

    // ---- C': the chunk backwards from its true end adjoint
    const double ln10_span = 2.302585092994045684 * (double)k.span;
    const double pi_sr = PS_PI / sr;
    const double depth_d = (double)depth[b];
    double a_dp = 0.0, a_ce = 0.0, a_fb = 0.0, a_mx = 0.0;
    {
        float L[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) L[c] = le[p * 8 + c];
        const int n_sub = (g1 - g0 + PS_SUB - 1) / PS_SUB;
        for (int sb = n_sub - 1; sb >= 0; --sb) {
            const int gs = g0 + sb * PS_SUB;
            const float4 *ck = st.ckpt(p, gpc, sb);
            const float4 c0 = ck[0], c1 = ck[1];
            float z[7] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z};
            float D[PB_S][6], O6[PB_S], GM[PB_S], Gs[PS_SUB];
            float mx32 = 0.0f;
            // the forward of the sub-block, JUCE's operation order (phaser.hip phase C)
#pragma unroll
            for (int u = 0; u < PS_SUB; ++u) {
                const int g = gs + u;
                const bool live = g < g1;
                const float G = live ? st.G()[g] : 0.0f;
                Gs[u] = G;
                float gm[4] = {0.f, 0.f, 0.f, 0.f};
                if (live) load_gm(g, gm);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = 4 * g + j, s = 4 * u + j;
                    const float in = (live && n < total) ? xb[n] : 0.0f;
                    const float out = ps_sample(G, fb, in, z, D[s]);
                    O6[s] = out;
                    GM[s] = gm[j];
                    mx32 = __builtin_fmaf(gm[j], out - in, mx32);
                }
            }
            a_mx += (double)mx32;
            // the adjoint over it
#pragma unroll
            for (int u = PS_SUB - 1; u >= 0; --u) {
                const int g = gs + u;
                if (g < g1) {
                    const float G = Gs[u];
                    float dG = 0.0f, fb32 = 0.0f;
#pragma unroll
                    for (int j = 3; j >= 0; --j) {
                        const int n = 4 * g + j, s = 4 * u + j;
                        fb32 = __builtin_fmaf(L[6], O6[s], fb32);
                        const float g_out = pb_adj_step<true>(L, G, GM[s], fb, wet_g, D[s], dG);
                        if (dxb && n < total) dxb[n] = __builtin_fmaf(k.dry_g, GM[s], g_out);
                    }
                    a_fb += (double)fb32;
                    // dG -> dlfo through G = g / (1 + g), g = tan(pi fc / sr), fc = 10^(lfo span + log_min), lfo = clip(pre)
                    const float pre = st.pre()[g];
                    double dlfo = 0.0;
                    if (pre >= 0.0f && pre <= 1.0f) {
                        const double Gd = (double)G, omG = 1.0 - Gd, gg = Gd / omG;
                        const double fc = pow(10.0, (double)__fadd_rn(__fmul_rn(pre, k.span), k.log_min));
                        dlfo = (double)dG * omG * omG * pi_sr * (1.0 + gg * gg) * fc * ln10_span;
                    }
                    a_dp += dlfo * 0.5 * (double)st.osc()[g];
                    a_ce += dlfo;
                    if (dmb && g < n_mod) dmb[g] = (float)(-dlfo * depth_d);
                }
            }
        }
    }
    // beyond the clip: zeros
    if (dxb)
        for (int n = total + p; n < x_width; n += PS_P) dxb[n] = 0.0f;
    if (dmb)
        for (int g = n_groups + p; g < n_mod; g += PS_P) dmb[g] = 0.0f;

    // ---- the four sums: per lane (above), butterfly, waves in order
    a_ce /= (double)centre[b] * ln10_span;
    const double s[4] = {a_dp, a_ce, a_fb, a_mx};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double t = wave_sum_f64(s[k]);
        if (lane == 0) red[k][p >> 6] = t;
    }
    __syncthreads();
    if (p < 4) {
        double t = 0.0;
        for (int i = 0; i < PS_WAVES; ++i) t += red[p][i];
        double *dst = p == 0 ? d_depth : p == 1 ? d_centre : p == 2 ? d_fb : d_mix;
        if (dst) dst[b] = t;
    }
}

// dy: row b at dy + b*dy_stride, N samples (the output window); x, x_stride, x_width, lead, rows / n_rows, B, N, sr and the
// per-clip parameters as given to mx_phaser_fwd_stash, whose stash (stash_groups, stash_stride) this reads.  Outputs, each
// optional: dx, row b at dx + b*dx_stride, x_width floats (zeros beyond lead[b] + N); dmod, row b at dmod + b*dmod_stride,
// n_mod floats (zeros beyond the clip's groups); d_depth, d_centre, d_feedback, d_mix (B,) fp64.
MX_EXPORT int mx_phaser_bwd(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, int64_t x_width,
                            const float *stash, int64_t stash_groups, int64_t stash_stride, const float *depth,
                            const float *centre, const float *feedback, const float *mix, const int32_t *lead,
                            const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, double sr, float *dx,
                            int64_t dx_stride, float *dmod, int64_t dmod_stride, int64_t n_mod, double *d_depth,
                            double *d_centre, double *d_feedback, double *d_mix, void *stream)
{
    if (!dy || !x || !stash || !depth || !centre || !feedback || !mix || B <= 0 || N <= 0 || sr <= 0.0) return MX_ERR_ARG;
    if (x_width < N || x_stride < x_width || dy_stride < N || (dx && dx_stride < x_width)) return MX_ERR_ARG;
    if (dmod && (n_mod < (x_width + 3) / 4 || dmod_stride < n_mod)) return MX_ERR_ARG;
    if (x_width >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    if (stash_groups < (x_width + 3) / 4 || (stash_groups & 3) || stash_stride < ps_stash_floats(stash_groups)) return MX_ERR_ARG;
    if ((stash_stride & 3) || ((uintptr_t)stash & 15)) return MX_ERR_ARG;      // the checkpoints are float4
    const int64_t items = rows ? n_rows : B;
    if (items <= 0) return MX_OK;
    const size_t lds = PS_LDS_FLOATS * sizeof(float);
    static MxLdsLatch latch = {};
    if (mx_set_dyn_lds(latch, (const void *)phaser_bwd_kernel, lds) != MX_OK) return MX_ERR_LAUNCH;
    hipLaunchKernelGGL(phaser_bwd_kernel, dim3((unsigned)items), dim3(PS_P), lds, (hipStream_t)stream, dy, (long long)dy_stride, x,
                       (long long)x_stride, (int)x_width, stash, (long long)stash_stride, (int)stash_groups, depth, centre,
                       feedback, mix, lead, rows, (int)N, sr, dx, (long long)dx_stride, dmod, (long long)dmod_stride,
                       dmod ? (int)n_mod : 0, d_depth, d_centre, d_feedback, d_mix);
    return mx_launch_status();
}
