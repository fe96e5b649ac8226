// phaser.hip -- K3: 6-stage all-pass phaser with feedback (reference call site:
// mod_extraction/datasets.py:455-482 -> pedalboard==0.7.3 Phaser == JUCE dsp::Phaser<float>;
// third-party source absent from the reference tree: PARITY UNPINNED, checked against
// oracle/csrc/oracle_ref.c:orc_phaser, which restates the published JUCE algorithm).
//
// Two kernels.  phaser_kernel: one wavefront per clip, every sample in JUCE's operation order, strictly serial -- the bit
// reference (exact_order != 0).  phaser_scan_kernel (default): the same recurrence as a linear scan over time, one
// workgroup per clip, one chunk of the clip per lane (see its header below).
// sin / pow / log10 are evaluated in fp64 and rounded once, which reproduces the host libm's (correctly rounded) float
// results; the LFO phase accumulator advances in fp32 exactly as JUCE's does.
// `lead` samples are processed (filter warm-up, LFO phase) before the N output samples: the
// reference renders n + sr/rate samples and crops at a random offset (datasets.py:428-449).
// Algorithmic HBM traffic: 8 B/sample (+4 B/sample when the cropped dry clip is also written).
#include "phaser_common.h"

#define PH_BLOCK 256
#define PH_WPB 4          // clips (wavefronts) per workgroup: packs the long-running serial chains onto few CUs so
                          // that the 1-workgroup-per-CU matrix kernels of the train step keep the other CUs

__global__ __launch_bounds__(64 * PH_WPB) void phaser_kernel(const float *__restrict__ x, long long x_stride,
                                                    const float *__restrict__ rate,
                                                    const float *__restrict__ depth,
                                                    const float *__restrict__ centre,
                                                    const float *__restrict__ feedback,
                                                    const float *__restrict__ mix,
                                                    const int *__restrict__ lead_arr,
                                                    const int *__restrict__ rows, int n_items, int N,
                                                    double sr, float *__restrict__ y, long long y_stride,
                                                    float *__restrict__ dry_out)
{
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * PH_WPB + (threadIdx.x >> 6);
    if (item >= n_items) return;                        // whole wave exits; waves never synchronise with each other
    const int b = rows ? rows[item] : item;
    const int lead = lead_arr ? lead_arr[b] : 0;
    const int total = lead + N;
    const float *xb = x + (size_t)b * x_stride;
    float *yb = y + (size_t)b * y_stride;
    float *db = dry_out ? dry_out + (size_t)b * y_stride : nullptr;

    const PsClip k = ps_clip(sr, rate[b], depth[b], centre[b], feedback[b], mix[b]);

    float phase = 0.0f;
    float z[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};            // s0..s5, lastOut

    for (int n0 = 0; n0 < total; n0 += PH_BLOCK) {
        // (1) coalesced load of 256 input samples: lane l holds samples n0 + j*64 + l, j = 0..3
        float xr[PH_BLOCK / 64], yr[PH_BLOCK / 64];
#pragma unroll
        for (int j = 0; j < PH_BLOCK / 64; ++j) {
            const int n = n0 + j * 64 + lane;
            xr[j] = n < total ? xb[n] : 0.0f;
            yr[j] = 0.0f;
        }
        // (2) sequential fp32 phase accumulation; lane k keeps the phase of update k
        float my_phase = 0.0f;
        for (int u = 0; u < PH_BLOCK / 4; ++u) {
            if (lane == u) my_phase = phase;
            phase = ps_step(phase, k.inc);
        }
        // (3) one cut-off update per lane: lane u holds G of samples 4u .. 4u+3 of this block
        float pre_unused;
        const float Greg = ps_cutoff(k, ps_osc(my_phase), pre_unused);
        // (4) the dependent chain, wave-uniform; inputs and coefficients are broadcast from lane
        //     registers (v_readlane) so that no LDS round trip sits between two samples
        const int cnt = min(PH_BLOCK, total - n0);
#pragma unroll
        for (int j = 0; j < PH_BLOCK / 64; ++j) {
            const int lim = min(64, cnt - j * 64);
            for (int li = 0; li < lim; ++li) {
                const float in = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xr[j]), li));
                const float G = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Greg), (j * 64 + li) >> 2));
                const float out = ps_sample(G, k.fb, in, z);
                float m = __fadd_rn(__fmul_rn(out, k.wet_g), __fmul_rn(in, k.dry_g));
                m = m < -1.0f ? -1.0f : (m > 1.0f ? 1.0f : m);
                yr[j] = lane == li ? m : yr[j];
            }
        }
        // (5) coalesced store of the samples that fall inside the output window
#pragma unroll
        for (int j = 0; j < PH_BLOCK / 64; ++j) {
            const int n = n0 + j * 64 + lane;
            if (n >= lead && n < total) {
                yb[n - lead] = yr[j];
                if (db) db[n - lead] = xr[j];
            }
        }
    }
}

// ---- the default kernel: the recurrence as a LINEAR SCAN over time -------------------------------------------------
// For a given cut-off sequence the phaser is a linear time-varying system in its 7-vector state z = (s0..s5, lastOut):
//     z(n+1) = A(G_n) z(n) + b(G_n) x(n).
// The cut-offs do not depend on the state (LFO only), so the clip is cut into PS_P = 512 chunks, one per LANE, and
//   A  every lane runs its chunk EIGHT times in registers -- from the seven unit states with silent input and from the
//      zero state with the real input -- which gives the chunk's affine map  z_end = M z_start + v  (the scalar all-pass
//      cascade costs 38 flops per sample and run; a dense 8 x 8 step would cost 128), and on the way evaluates its
//      cut-off updates (one fp64 sin / pow / tan per 4 samples: each update of the clip is still evaluated exactly once)
//      and parks them in a workspace;
//   B  seven lanes of one wave chain the 512 maps (a 7 x 7 mat-vec per chunk, ~25 us): the state at every chunk start;
//   C  every lane re-runs its chunk from its true start state in JUCE's operation order and writes the output window.
// No sample waits for its predecessor outside a chunk of ~345: 85 clips x (2 s + lead) take ~0.4 ms where the
// state-space step on a producer / consumer wave pair (round 2, one dependent 8 x 8 step per sample) took 7.8 ms.
// Rounding: phase C is the reference's own arithmetic; only the chunk-start states carry the re-association error of the
// maps (~1e-7 of the state, it decays like any state perturbation of the stable all-pass loop).
// The LFO phase at a chunk start must equal what 44 100 sequential fp32 additions give (JUCE accumulates in fp32; a
// closed form in fp64 is 1e-5 rad off after a few thousand steps): ps_phase_after() below reproduces them exactly in
// O(binades) steps.
// (PS_P, PS_MV, PS_LDS_FLOATS: phaser_common.h)
//
// STASH = true (mx_phaser_fwd_stash) is the forward of the adjoint in phaser_bwd.hip: the same scan, y bit-identical, that
//  * may take the LFO from outside: `mod`, one value in [0, 1] per cut-off update, osc = 1 - 2 mod in place of
//    sin(phase - pi) (the rate is then not read).  The sign makes mod the reference's phaser ground truth
//    make_mod_signal(.., pi / 2, "cos") = (cos(wt + pi / 2 + pi) + 1) / 2 = (1 + sin wt) / 2 (modulations.py:35,
//    datasets.py:442), since JUCE's sin(phase - pi) = -sin(phase);
//  * leaves per group G, pre (the lfo before its clamp), osc and the four output-clip decisions, per chunk the map M of
//    phase A (its transpose is the chunk map of the adjoint: the backward does not run seven unit adjoints), and the state
//    at the start of every PS_SUB-th group (phase C), from which the backward recomputes 8 samples at a time in registers.
// Both instantiations share their arithmetic with phaser_kernel and the adjoint through phaser_common.h.  What keeps
// STASH = false the plain forward is checked on the device assembly whenever this code is restructured: the same VGPR /
// SGPR counts, no scratch, and the same count of every fp32 / fp64 arithmetic opcode as before (instruction order and
// register numbering may differ), and bit-equal outputs on the timing tools' draws.

// phase after g cut-off updates:  p <- fl(p + inc);  while (p >= 2 pi) p <- fl(p - 2 pi)   (oracle_ref.c:orc_phaser)
// Inside one binade [2^e, 2^(e+1)) every representable p is a multiple of ulp = 2^(e-23), so fl(p + inc) = p + d with ONE
// constant d = rn(inc / ulp) ulp -- except that a tie (inc / ulp = I + 1/2 exactly) rounds to even and can make the FIRST
// step from an odd multiple differ from all later ones.  Hence: three real steps; if the last two are equal and all
// three values share a binade, jump  p += j d  (exact in fp32: stays inside the binade, below 2 pi, one step of margin),
// then continue with real steps across the binade edge / the wrap.  ~25 rounds per LFO period; checked against the
// sequential loop for 600 (rate, count) pairs including constructed ties (tools/probe/check_phase_jump.py).
__device__ float ps_phase_after(int g, float inc)
{
    const float two_pi = PS_TWO_PI;
    float p = 0.0f;
    int rem = g;
    while (rem > 0) {
        const float p1 = ps_step(p, inc);
        p = p1;
        if (--rem == 0) break;
        const float p2 = ps_step(p1, inc);
        p = p2;
        if (--rem == 0) break;
        const float p3 = ps_step(p2, inc);
        p = p3;
        if (--rem == 0) break;
        const float d1 = __fsub_rn(p2, p1), d2 = __fsub_rn(p3, p2);
        const int e1 = (__float_as_int(p1) >> 23) & 0xff, e2 = (__float_as_int(p2) >> 23) & 0xff, e3 = (__float_as_int(p3) >> 23) & 0xff;
        if (d1 == d2 && d2 > 0.0f && e1 == e2 && e2 == e3 && e3 > 0 && e3 < 0xfe) {
            const double edge = (double)__int_as_float((e3 + 1) << 23);          // 2^(e+1)
            const double lim = edge < (double)two_pi ? edge : (double)two_pi;
            long long j = (long long)floor((lim - (double)p3) / (double)d2) - 1;
            if (j > rem) j = rem;
            if (j > 0) {
                p = (float)((double)p3 + (double)j * (double)d2);
                rem -= (int)j;
            }
        }
    }
    return p;
}

template <bool STASH>
__global__ __launch_bounds__(PS_P) void phaser_scan_kernel(const float *__restrict__ x, long long x_stride,
                                                           const float *__restrict__ rate,
                                                           const float *__restrict__ depth,
                                                           const float *__restrict__ centre,
                                                           const float *__restrict__ feedback,
                                                           const float *__restrict__ mix,
                                                           const int *__restrict__ lead_arr,
                                                           const int *__restrict__ rows, int n_items, int N, double sr,
                                                           float *__restrict__ y, long long y_stride,
                                                           float *__restrict__ dry_out, float *__restrict__ gws,
                                                           long long gws_stride, int probe,
                                                           const float *__restrict__ mod, long long mod_stride, int n_mod,
                                                           float *__restrict__ stash, long long stash_stride, int sg,
                                                           int x_width)
{
    extern __shared__ __attribute__((aligned(16))) float ps_lds[];
    float *mv = ps_lds, *zs = ps_lds + PS_P * PS_MV;
    const int p = threadIdx.x, lane = p & 63;
    const int item = blockIdx.x;
    const int b = rows ? rows[item] : item;
    const int lead = lead_arr ? lead_arr[b] : 0;
    const int total = lead + N;
    const float *xb = x + (size_t)b * x_stride;
    float *yb = y + (size_t)b * y_stride;
    float *db = dry_out ? dry_out + (size_t)b * y_stride : nullptr;
    float *gw = gws + (size_t)item * gws_stride;
    // STASH: the group records double as the cut-off workspace; a clip that does not fit its row is left alone
    PsStash<float> st = {nullptr, sg};
    const float *mb = nullptr;
    if constexpr (STASH) {
        if (total > x_width || ((total + 3) >> 2) > sg) return;
        st.row = stash + (size_t)b * stash_stride;
        gw = st.G();
        if (mod) mb = mod + (size_t)b * mod_stride;
    }
    const bool ext = STASH && mb != nullptr;                     // the LFO comes from outside

    const PsClip k = ps_clip(sr, ext ? 0.0f : rate[b], depth[b], centre[b], feedback[b], mix[b]);

    const int n_groups = (total + 3) >> 2;                       // cut-off updates = groups of 4 samples from sample 0
    const int gpc = (n_groups + PS_P - 1) / PS_P;                // groups per chunk
    const int g0 = p * gpc, g1 = min(g0 + gpc, n_groups);        // this lane's groups [g0, g1) (empty beyond the clip)

    const bool use_ws = STASH || (gws != nullptr && (long long)n_groups <= gws_stride);

    // ---- A: the chunk's affine map, the cut-offs on the way
    float S[8][7];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 7; ++c) S[r][c] = r == c ? 1.0f : 0.0f;
    float phase = ext ? 0.0f : ps_phase_after(min(g0, n_groups), k.inc);
    for (int g = g0; g < g1; ++g) {
        float xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 4 * g + j;
            xv[j] = probe ? 0.25f : (n < total ? xb[n] : 0.0f);
        }
        float pre;
        const float osc = ext ? __fsub_rn(1.0f, __fmul_rn(2.0f, g < n_mod ? mb[g] : 0.5f)) : ps_osc(phase);
        const float G = ps_cutoff(k, osc, pre);
        if constexpr (STASH) {
            st.pre()[g] = pre;
            st.osc()[g] = osc;
        }
        phase = ps_step(phase, k.inc);
        if (use_ws) gw[g] = G;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int r = 0; r < 8; ++r) (void)ps_sample(G, k.fb, r == 7 ? xv[j] : 0.0f, S[r]);
        }
    }
    {
        float *m = mv + p * PS_MV;
#pragma unroll
        for (int c = 0; c < 7; ++c)
#pragma unroll
            for (int r = 0; r < 7; ++r) m[c * 7 + r] = S[c][r];      // column c = image of unit state c
#pragma unroll
        for (int r = 0; r < 7; ++r) m[49 + r] = S[7][r];
        if constexpr (STASH) m[PS_MV - 1] = 0.0f;                // the pad float goes into the stash with the map
    }
    __syncthreads();

    // ---- B: chain the maps (wave 0; lane r < 7 owns row r, the new state is broadcast with v_readlane)
    if (p < 64) {
        const int r = lane < 7 ? lane : 0;
        float z[7], mine = 0.0f;
#pragma unroll
        for (int c = 0; c < 7; ++c) z[c] = 0.0f;
        for (int q = 0; q < PS_P; ++q) {
            if (lane < 7) zs[q * 8 + lane] = mine;
            const float *m = mv + q * PS_MV;
            float acc = m[49 + r];
#pragma unroll
            for (int c = 0; c < 7; ++c) acc = __builtin_fmaf(m[c * 7 + r], z[c], acc);
            mine = acc;
#pragma unroll
            for (int c = 0; c < 7; ++c) z[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), c));
        }
    }
    __syncthreads();
    if constexpr (STASH) {                                       // the chunk maps, as they lie in LDS
        for (int i = p; i < PS_P * PS_MV; i += PS_P) st.maps()[i] = mv[i];
        // Every word of the row's ps_stash_floats(sg) that the scan does not write is zeroed, so a stash row never carries what
        // its allocation held: the group records beyond the clip, this chunk's checkpoint slots without a group, and the
        // checkpoints beyond the clip's own packing (the row is laid out for sg groups, the clip packs n_groups <= sg).
        for (int g = n_groups + p; g < sg; g += PS_P) {
            st.G()[g] = 0.0f;
            st.pre()[g] = 0.0f;
            st.osc()[g] = 0.0f;
            st.pass()[g] = 0;
        }
        const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const int spc = (gpc + PS_SUB - 1) / PS_SUB;
        for (int sub = (max(g1 - g0, 0) + PS_SUB - 1) / PS_SUB; sub < spc; ++sub) {
            float4 *ck = st.ckpt(p, gpc, sub);
            ck[0] = zero4;
            ck[1] = zero4;
        }
        float4 *ck_all = st.ckpt(0, gpc, 0);
        const long long ck_used = 2ll * PS_P * spc, ck_row = 2ll * PS_P * ps_ckpts_per_chunk(sg);
        for (long long i = ck_used + p; i < ck_row; i += PS_P) ck_all[i] = zero4;
    }

    // ---- C: the chunk from its true start state, JUCE's operation order, output window
    {
        float z[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) z[c] = zs[p * 8 + c];
        float phase_c = use_ws ? 0.0f : ps_phase_after(min(g0, n_groups), k.inc);
        for (int g = g0; g < g1; ++g) {
            float G;
            if (use_ws) G = gw[g];
            else {                                               // workspace too small for this clip: evaluate the cut-off again
                float pre_unused;
                G = ps_cutoff(k, ps_osc(phase_c), pre_unused);
                phase_c = ps_step(phase_c, k.inc);
            }
            float xv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = 4 * g + j;
                xv[j] = probe ? 0.25f : (n < total ? xb[n] : 0.0f);
            }
            int passed = 0;
            if constexpr (STASH) {
                if (((g - g0) & (PS_SUB - 1)) == 0) {
                    float4 *ck = st.ckpt(p, gpc, (g - g0) / PS_SUB);
                    ck[0] = make_float4(z[0], z[1], z[2], z[3]);
                    ck[1] = make_float4(z[4], z[5], z[6], 0.0f);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = 4 * g + j;
                const float in = xv[j];
                const float out = ps_sample(G, k.fb, in, z);
                float m = __fadd_rn(__fmul_rn(out, k.wet_g), __fmul_rn(in, k.dry_g));
                if constexpr (STASH) passed |= (m >= -1.0f && m <= 1.0f) ? 1 << j : 0;
                m = m < -1.0f ? -1.0f : (m > 1.0f ? 1.0f : m);
                if (n >= lead && n < total && (!probe || g + 1 == g1)) {
                    yb[n - lead] = m;
                    if (db) db[n - lead] = in;
                }
            }
            if constexpr (STASH) st.pass()[g] = passed;
        }
    }
}

// x: source audio, row b at x + b*x_stride, at least lead[b] + N samples; rate, depth, centre,
// feedback, mix: (B,) fp32; lead: (B,) int32 warm-up samples (NULL = 0); rows/n_rows: optional
// subset of clip indices.  y: row b at y + b*y_stride, N samples = processed[lead : lead+N];
// dry_out (optional, same stride as y): the matching crop of the source.
// exact_order != 0: the whole clip sample by sample on one wavefront in JUCE's operation order (the bit reference);
// 0: the time-parallel linear scan above.  workspace: floats, row `item` at workspace + item * workspace_stride, at least
// ceil((lead + N) / 4) floats per processed clip (the cut-off of every 4-sample group, kept between the two passes of
// the scan); optional: NULL or too short a row makes the kernel evaluate the cut-offs twice instead.
static int phaser_fwd_launch(const float *x, int64_t x_stride, const float *rate, const float *depth,
                            const float *centre, const float *feedback, const float *mix, const int32_t *lead,
                            const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, double sr, int32_t exact_order,
                            float *y, int64_t y_stride, float *dry_out, float *workspace, int64_t workspace_stride,
                            void *stream, int probe)
{
    if (!x || !rate || !depth || !centre || !feedback || !mix || !y || B <= 0 || N <= 0 || sr <= 0.0) return MX_ERR_ARG;
    if (workspace && workspace_stride <= 0) return MX_ERR_ARG;
    if (N >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    const int64_t items = rows ? n_rows : B;
    if (items <= 0) return MX_OK;
    if (exact_order) {
        const dim3 grid((unsigned)((items + PH_WPB - 1) / PH_WPB)), block(64 * PH_WPB);
        hipLaunchKernelGGL(phaser_kernel, grid, block, 0, (hipStream_t)stream, x, (long long)x_stride, rate, depth, centre,
                           feedback, mix, lead, rows, (int)items, (int)N, sr, y, (long long)y_stride, dry_out);
    } else {
        const size_t lds = PS_LDS_FLOATS * sizeof(float);
        static MxLdsLatch latch = {};
        if (mx_set_dyn_lds(latch, (const void *)phaser_scan_kernel<false>, lds) != MX_OK) return MX_ERR_LAUNCH;
        hipLaunchKernelGGL(phaser_scan_kernel<false>, dim3((unsigned)items), dim3(PS_P), lds, (hipStream_t)stream, x, (long long)x_stride,
                           rate, depth, centre, feedback, mix, lead, rows, (int)items, (int)N, sr, y, (long long)y_stride,
                           dry_out, workspace, (long long)workspace_stride, probe, (const float *)nullptr, 0ll, 0,
                           (float *)nullptr, 0ll, 0, 0);
    }
    return mx_launch_status();
}

MX_EXPORT int mx_phaser_fwd(const float *x, int64_t x_stride, const float *rate, const float *depth,
                            const float *centre, const float *feedback, const float *mix, const int32_t *lead,
                            const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, double sr, int32_t exact_order,
                            float *y, int64_t y_stride, float *dry_out, float *workspace, int64_t workspace_stride,
                            void *stream)
{
    return phaser_fwd_launch(x, x_stride, rate, depth, centre, feedback, mix, lead, rows, n_rows, B, N, sr, exact_order, y, y_stride, dry_out, workspace, workspace_stride, stream, 0);
}

// Forward of the adjoint (phaser_bwd.hip): the scan with STASH, see the kernel's header.  x_width: valid floats of an x row
// (a clip whose lead + N exceeds it is SKIPPED: outputs untouched, status MX_OK -- lead is device data, the caller keeps
// the contract); mod (optional): row b at mod + b*n_mod, n_mod >= ceil(x_width / 4) values in [0, 1], rate may then be NULL;
// stash: 16-byte aligned, row b at stash + b*stash_stride (a multiple of 4), laid out for stash_groups groups
// (phaser_common.h), stash_groups a multiple of 4 and >= ceil(x_width / 4).
MX_EXPORT int mx_phaser_fwd_stash(const float *x, int64_t x_stride, int64_t x_width, const float *mod, int64_t n_mod,
                                  const float *rate, const float *depth, const float *centre, const float *feedback,
                                  const float *mix, const int32_t *lead, const int32_t *rows, int64_t n_rows, int64_t B,
                                  int64_t N, double sr, float *y, int64_t y_stride, float *dry_out, float *stash,
                                  int64_t stash_groups, int64_t stash_stride, void *stream)
{
    if (!x || !(mod || rate) || !depth || !centre || !feedback || !mix || !y || !stash || B <= 0 || N <= 0 || sr <= 0.0)
        return MX_ERR_ARG;
    if (x_width < N || x_stride < x_width || y_stride < N || (mod && n_mod < (x_width + 3) / 4)) return MX_ERR_ARG;
    if (x_width >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    if (stash_groups < (x_width + 3) / 4 || (stash_groups & 3) || stash_stride < ps_stash_floats(stash_groups)) return MX_ERR_ARG;
    if ((stash_stride & 3) || ((uintptr_t)stash & 15)) return MX_ERR_ARG;      // the checkpoints are float4
    const int64_t items = rows ? n_rows : B;
    if (items <= 0) return MX_OK;
    const size_t lds = PS_LDS_FLOATS * sizeof(float);
    static MxLdsLatch latch = {};
    if (mx_set_dyn_lds(latch, (const void *)phaser_scan_kernel<true>, lds) != MX_OK) return MX_ERR_LAUNCH;
    hipLaunchKernelGGL(phaser_scan_kernel<true>, dim3((unsigned)items), dim3(PS_P), lds, (hipStream_t)stream, x, (long long)x_stride,
                       rate, depth, centre, feedback, mix, lead, rows, (int)items, (int)N, sr, y, (long long)y_stride, dry_out,
                       (float *)nullptr, 0ll, 0, mod, (long long)n_mod, (int)n_mod, stash, (long long)stash_stride,
                       (int)stash_groups, (int)x_width);
    return mx_launch_status();
}

// Measurement twin (bench.py's serial floor): the SAME launch with no global-memory traffic inside the sample loop -- inputs are constants, only the last chunk is stored.  Results are meaningless; nothing in the product calls it.
MX_EXPORT int mx_phaser_fwd_probe(const float *x, int64_t x_stride, const float *rate, const float *depth,
                            const float *centre, const float *feedback, const float *mix, const int32_t *lead,
                            const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, double sr, int32_t exact_order,
                            float *y, int64_t y_stride, float *dry_out, float *workspace, int64_t workspace_stride,
                            void *stream)
{
    return phaser_fwd_launch(x, x_stride, rate, depth, centre, feedback, mix, lead, rows, n_rows, B, N, sr, exact_order, y, y_stride, dry_out, workspace, workspace_stride, stream, 1);
}

// ---- independent floor of the scan (bench.py) -----------------------------------------------------------
// `mx_phaser_fwd_probe` re-runs the product kernel without global traffic: that floor inherits its schedule.  This
// microbenchmark is nothing but the arithmetic NO schedule of the scan can avoid: the 6-stage all-pass cascade of one sample
// (JUCE's FirstOrderTPTFilter step x 6 + feedback, 38 flops) for EIGHT independent state vectors per lane -- the shape of
// phase A (seven unit states + the driven zero state) -- on one 512-lane workgroup, with a constant cut-off and input: no loads,
// no stores, no fp64 sin / pow / tan, no chunk maps, no chaining.  time / (steps x 8) = the cost of one (sample, run) at the
// kernel's occupancy; a clip needs ceil((lead + N) / 512) samples per lane x 9 runs (8 of phase A + phase C).
__global__ __launch_bounds__(PS_P) void phaser_cascade_probe_kernel(int steps, float G, float fb, float *__restrict__ out)
{
    float s[8][6], last[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        last[r] = 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[r][k] = (r == k) ? 1.0f : 0.001f * (float)(threadIdx.x & 7);
    }
    float in = 0.25f + 1e-3f * (float)(threadIdx.x & 15);
    for (int t = 0; t < steps; ++t) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float o = __fsub_rn(r == 7 ? in : 0.0f, last[r]);
#pragma unroll
            for (int k = 0; k < 6; ++k) (void)ps_stage(G, s[r][k], o);
            last[r] = __fmul_rn(o, fb);
        }
        in = -in;
    }
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) acc += last[r] + s[r][5];
    if (acc == 123.456f) out[threadIdx.x] = acc;             // keeps the chains live; never true for these constants
    if (threadIdx.x == 0) out[0] = acc;
}

// `steps` samples x 8 independent cascade runs per lane on one 512-lane workgroup (see above); out: >= 512 floats
MX_EXPORT int mx_phaser_cascade_probe(int64_t steps, float *out, void *stream)
{
    if (!out || steps <= 0 || steps >= (1ll << 30)) return MX_ERR_ARG;
    hipLaunchKernelGGL(phaser_cascade_probe_kernel, dim3(1), dim3(PS_P), 0, (hipStream_t)stream, (int)steps, 0.37f, 0.45f, out);
    return mx_launch_status();
}
