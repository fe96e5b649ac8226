// flanger_bwd.hip -- K2 adjoint: gradient of the mono flanger / chorus (reference: mod_extraction/fx.py:72-119) with
// respect to x, mod_sig and the per-clip constants, from the taps v[n] that mx_flanger_fwd_stash (flanger.hip) stored.
//
// The gradient is the derivative of the reference loop restated without in-place writes: floor (prev / next) has zero
// derivative, the read fraction and torch.remainder derivative 1, clip passes the gradient where -1 <= z <= 1, and slots
// read before they were ever written read 0 (gradient sent there is dropped).  Per sample n (v the tap, d = x + fb v the
// value written, o = x + depth v, z = (1-mix) x + mix o):
//   g_z = dy [-1 <= z <= 1],  g_o = mix g_z,  g_v = depth g_o + fb g_d,
//   g_d[n] = sum over the later reads of d[n] of their interpolation weight x g_v   (reverse-time recurrence)
//   dx = (1-mix) g_z + g_o + g_d,  g_f = g_v (d[next] - d[prev]),  dmod = -lfo_scale g_f
//   d feedback = sum g_d v, d depth = sum g_o v, d mix = sum g_z (o - x), d lfo_scale = -sum g_f mod, d min_delay = -sum g_f
//
// Two launches.
//  1. fb_recur_kernel -- the serial part, g_d.  One workgroup = one clip = a consumer wave + FL_V producer waves, as in
//     the forward, walking the clip BACKWARDS in chunks of 512 samples.  An LDS accumulator A[M] is indexed like the
//     delay line: A[s] holds the gradient already sent to the value slot s currently holds.  Reverse of one sample
//     (read prev / next, then write w): g_d = A[w], A[w] = 0; then A[prev] += (1-f) g_v, A[next] += f g_v.  The forward's
//     dependency-free runs (no read of a run sees a write of the same run) are valid lock-steps of this reverse sweep: the
//     whole run takes its g_d first, then scatters.  The producers additionally split a run where the age of the value
//     read at prev (or at next) does not increase from one sample to the next: inside a dependency-free run equal slots
//     mean equal ages, so every scatter instruction of a lock-step has pairwise distinct addresses (one ds_add_f32 for all
//     prev halves, then one for all next halves; LDS executes one wave's instructions in order).  No two lanes ever race on
//     an address, so the sums are the same on every run.
//  2. fb_out_kernel -- everything else is independent per sample: one workgroup per clip recomputes the slots, z and the
//     two values d read (x and the stash at most M samples back, L2-resident), writes dx and dmod, and sums the five
//     parameter partials in fp64 in a fixed order (per thread, then a butterfly, then the waves in order).
//
// LR = true (mx_flanger_bwd_lr): the LFO is the low-rate row (B, n_mod < N) the forward resampled in-kernel.  Both kernels
// recompute a sample's LFO value with the forward's own fl_lfo (flanger_common.h), so slots, fractions and runs are the
// forward's; fb_recur_kernel keeps the row in LDS behind A, as the forward keeps it behind the delay line.  dmod is
// (B, n_mod): the transpose of the resampling applied to the per-sample -lfo_scale g_f.  fb_out_kernel owns the clip, so
// the thread of sample n overwrites ws[n] (the g_d it has just consumed) with that value, and after a workgroup fence
// and barrier one wave per low-rate point gathers the contiguous range of samples that have a tap on the point: lanes
// stride the range, weights are interp_tap's fp32 taps, products and sums fp64 in a fixed order (per lane, then a
// butterfly), rounded once.  No (B, N) buffer beyond ws, no atomics.
#include "flanger_common.h"     // the forward's geometry, fl_slots, fl_dist, fl_run_masks, the slot word

#define FB_OUT_THREADS 512

// the forward's output z (fx.py:115-117, before the clip) and o, recomputed bit-exactly from x and the tap
__device__ __forceinline__ float fb_z(float xv, float v, float dp, float mx, float omm, float &o)
{
    o = __fadd_rn(xv, __fmul_rn(dp, v));
    return __fadd_rn(__fmul_rn(omm, xv), __fmul_rn(mx, o));
}

template <bool LR>
__global__ __launch_bounds__(FL_THREADS) void fb_recur_kernel(
    const float *__restrict__ dy, long long dy_stride, const float *__restrict__ x, long long x_stride,
    const float *__restrict__ mod, const float *__restrict__ stash, const float *__restrict__ lfo_scale,
    const float *__restrict__ min_delay, const float *__restrict__ feedback, const float *__restrict__ depth,
    const float *__restrict__ mix, const float *__restrict__ one_minus_mix, const int *__restrict__ max_delay,
    const int *__restrict__ rows, int N, int n_mod, float mod_scale, int lfo_off, int ring_off, float *__restrict__ gd_out)
{
    extern __shared__ __attribute__((aligned(16))) float buf[];        // [A: M floats | LR: n_mod LFO row | ring]
    const int lane = threadIdx.x & 63;
    const bool producer = threadIdx.x >= 64;
    const int pw = (int)(threadIdx.x >> 6) - 1;
    const int b = rows ? rows[blockIdx.x] : (int)blockIdx.x;
    const int M = max_delay[b];
    const float Mf = (float)M;
    const float ls = lfo_scale[b], md = min_delay[b], fb = feedback[b], dp = depth[b];
    const float mx = mix[b], omm = one_minus_mix[b];
    const float *dyb = dy + (size_t)b * dy_stride;
    const float *xb = x + (size_t)b * x_stride;
    const float *mb = mod + (size_t)b * (LR ? n_mod : N);
    const float *sb = stash + (size_t)b * N;
    float *gb = gd_out + (size_t)b * N;
    float *ring = buf + ring_off;
    const float *lfo = buf + lfo_off;

    for (int i = threadIdx.x; i < M; i += FL_THREADS) buf[i] = 0.0f;
    if (LR) {
        for (int i = threadIdx.x; i < n_mod; i += FL_THREADS) buf[lfo_off + i] = mb[i];
        __syncthreads();                                               // the producers read the row before the first barrier
    }

    const int n_chunks = (N + FL_CHUNK - 1) / FL_CHUNK;
    // producer: inputs of the chunk it builds next, loaded one chunk ahead
    float xr = 0.0f, mr = 0.0f, vr = 0.0f, gr = 0.0f;
    auto load = [&](int c) {
        const int n = c * FL_CHUNK + pw * 64 + lane;
        const bool ok = c >= 0 && n < N;
        xr = ok ? xb[n] : 0.0f;
        mr = ok && !LR ? mb[n] : 0.0f;
        vr = ok ? sb[n] : 0.0f;
        gr = ok ? dyb[n] : 0.0f;
    };
    // records of row pw of chunk c -> ring slot c & 1: {depth g_o, f, 1 - f, w | prev << 16} and the lane masks of the
    // row's lock-steps (run r in lane r)
    auto build = [&](int c) {
        const int n = c * FL_CHUNK + pw * 64 + lane;
        const FlSlot slot = fl_slot(ring, c);
        const float xv = xr, v = vr, g = gr;
        const bool valid = n < N;
        const float m = LR ? fl_lfo(lfo, mod_scale, valid ? n : 0, n_mod) : mr;
        load(c - 1);
        const int w = valid ? n % M : 0;
        int prev, next;
        float frac;
        fl_slots(w, m, ls, md, M, Mf, prev, next, frac);
        float o;
        const float z = fb_z(xv, v, dp, mx, omm, o);
        const float gz = (z >= -1.0f && z <= 1.0f) ? g : 0.0f;         // clamp's backward: inclusive bounds
        const float gvo = valid ? __fmul_rn(dp, __fmul_rn(mx, gz)) : 0.0f;
        slot.rec[pw * 64 + lane] = make_float4(gvo, frac, __fsub_rn(1.0f, frac), fl_pack(w, prev));
        const int dpr = fl_dist(w, prev, M), dnx = fl_dist(w, next, M);
        const int dep = min(dpr, dnx);
        int tk = !valid || dep > lane ? -1 : lane - dep;               // newest sample of this row the reads depend on
        // ages of the two values read; inside a dependency-free run equal slots <=> equal ages: split where an age does
        // not increase, so that the scatter addresses of a lock-step are distinct
        const int age_p = n - dpr, age_n = n - dnx;
        const int age_p1 = __shfl_up(age_p, 1, 64), age_n1 = __shfl_up(age_n, 1, 64);
        if (valid && lane > 0 && (age_p <= age_p1 || age_n <= age_n1)) tk = max(tk, lane - 1);
        int run;
        slot.run_mask[pw * 64 + lane] = fl_run_masks(lane, tk, __ballot(valid), run);
        if (lane == 0) slot.n_runs[pw] = run;
    };

    if (producer) {
        load(n_chunks - 1);
        build(n_chunks - 1);
    }
    for (int c = n_chunks - 1; c >= 0; --c) {
        __syncthreads();                                               // records of chunk c complete; slot (c - 1) & 1 free
        if (producer) {
            if (c > 0) build(c - 1);
        } else {
            const FlSlot slot = fl_slot(ring, c);
            float gd_[FL_V];
#pragma unroll
            for (int j = FL_V - 1; j >= 0; --j) {
                const float4 rc = slot.rec[j * 64 + lane];
                const unsigned long long m64 = slot.run_mask[j * 64 + lane];
                const unsigned m_lo = (unsigned)m64, m_hi = (unsigned)(m64 >> 32);
                const int nr = __builtin_amdgcn_readfirstlane(slot.n_runs[j]);
                int w, prev, next;
                fl_unpack(rc.w, M, w, prev, next);
                const float gvo = rc.x, frac = rc.y, omf = rc.z;
                float gd = 0.0f;
                for (int r = nr - 1; r >= 0; --r) {
                    // (readlane returns int: zero-extend the low half, or bit 31 would set lanes 32-63)
                    const unsigned long long msk = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(m_hi, r) << 32) |
                                                   (unsigned)__builtin_amdgcn_readlane(m_lo, r);
                    asm volatile("" ::: "memory");                     // keep this lock-step's LDS traffic behind the last
                    if ((msk >> lane) & 1ull) {
                        gd = __hip_atomic_exchange(buf + w, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const float gv = __fadd_rn(gvo, __fmul_rn(fb, gd));
                        __hip_atomic_fetch_add(buf + prev, __fmul_rn(omf, gv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        asm volatile("" ::: "memory");                 // all prev halves, then all next halves
                        __hip_atomic_fetch_add(buf + next, __fmul_rn(frac, gv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                gd_[j] = gd;
            }
#pragma unroll
            for (int j = 0; j < FL_V; ++j) {
                const int n = c * FL_CHUNK + j * 64 + lane;
                if (n < N) gb[n] = gd_[j];
            }
        }
    }
}

template <bool LR>
__global__ __launch_bounds__(FB_OUT_THREADS) void fb_out_kernel(
    const float *__restrict__ dy, long long dy_stride, const float *__restrict__ x, long long x_stride,
    const float *__restrict__ mod, int n_mod, float mod_scale, const float *__restrict__ stash, float *ws,
    const float *__restrict__ lfo_scale, const float *__restrict__ min_delay, const float *__restrict__ feedback,
    const float *__restrict__ depth, const float *__restrict__ mix, const float *__restrict__ one_minus_mix,
    const int *__restrict__ max_delay, const int *__restrict__ rows, int N, float *__restrict__ dx, long long dx_stride,
    float *__restrict__ dmod, long long dmod_stride, double *__restrict__ d_ls, double *__restrict__ d_md,
    double *__restrict__ d_fb, double *__restrict__ d_dp, double *__restrict__ d_mx)
{
    __shared__ double red[5][FB_OUT_THREADS / 64];
    const int b = rows ? rows[blockIdx.x] : (int)blockIdx.x;
    const int M = max_delay[b];
    const float Mf = (float)M;
    const float ls = lfo_scale[b], md = min_delay[b], fb = feedback[b], dp = depth[b];
    const float mx = mix[b], omm = one_minus_mix[b];
    const float *dyb = dy + (size_t)b * dy_stride;
    const float *xb = x + (size_t)b * x_stride;
    const float *mb = mod + (size_t)b * (LR ? n_mod : N);
    const float *sb = stash + (size_t)b * N;
    float *gb = ws + (size_t)b * N;                                    // g_d in; LR: the per-sample -lfo_scale g_f out
    double s_ls = 0.0, s_md = 0.0, s_fb = 0.0, s_dp = 0.0, s_mx = 0.0;
    for (int n = threadIdx.x; n < N; n += FB_OUT_THREADS) {
        const float xv = xb[n], v = sb[n], g = dyb[n], gd = gb[n];
        const float m = LR ? fl_lfo(mb, mod_scale, n, n_mod) : mb[n];
        const int w = n % M;
        int prev, next;
        float frac;
        fl_slots(w, m, ls, md, M, Mf, prev, next, frac);
        float o;
        const float z = fb_z(xv, v, dp, mx, omm, o);
        const double gz = (z >= -1.0f && z <= 1.0f) ? (double)g : 0.0;
        const double go = (double)mx * gz;
        const double gv = (double)dp * go + (double)fb * (double)gd;
        // the two values the reads of step n saw: d of the last write of each slot before n (0 if never written)
        const int mp = n - fl_dist(w, prev, M), mn = n - fl_dist(w, next, M);
        const float d_p = mp >= 0 ? __fadd_rn(xb[mp], __fmul_rn(fb, sb[mp])) : 0.0f;
        const float d_n = mn >= 0 ? __fadd_rn(xb[mn], __fmul_rn(fb, sb[mn])) : 0.0f;
        const double gf = gv * ((double)d_n - (double)d_p);
        if (dx) dx[(size_t)b * dx_stride + n] = (float)((double)omm * gz + go + (double)gd);
        if (dmod) (LR ? gb : dmod + (size_t)b * dmod_stride)[n] = (float)(-(double)ls * gf);
        s_ls += gf * (double)m;
        s_md += gf;
        s_fb += (double)gd * (double)v;
        s_dp += go * (double)v;
        s_mx += gz * ((double)o - (double)xv);
    }
    const double s[5] = {s_ls, s_md, s_fb, s_dp, s_mx};
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double t = wave_sum_f64(s[k]);
        if ((threadIdx.x & 63) == 0) red[k][wv] = t;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        double t = 0.0;
        for (int i = 0; i < FB_OUT_THREADS / 64; ++i) t += red[k][i];
        double *dst = k == 0 ? d_ls : k == 1 ? d_md : k == 2 ? d_fb : k == 3 ? d_dp : d_mx;
        if (dst) dst[b] = k < 2 ? -t : t;
    }
    if (LR && dmod) {
        __threadfence_block();                                         // every sample's value is in ws before any is gathered
        __syncthreads();
        const int lane = threadIdx.x & 63;
        for (int k = wv; k < n_mod; k += FB_OUT_THREADS / 64) {
            // point k is tap i0 of the samples with i0 == k and tap i1 of those with i0 == k - 1; i0 does not decrease with
            // n, so they form one range.  Its first sample from an estimate, corrected with the forward's own taps.
            int n0 = 0;
            if (k > 0) {
                n0 = (int)fminf((float)(k - 1) / mod_scale, (float)(N - 1));
                while (n0 > 0 && interp_tap(mod_scale, n0 - 1, n_mod).i0 >= k - 1) --n0;
                while (n0 < N && interp_tap(mod_scale, n0, n_mod).i0 < k - 1) ++n0;
            }
            double acc = 0.0;
            for (int n = n0 + lane; n < N; n += 64) {
                const InterpTap t = interp_tap(mod_scale, n, n_mod);
                if (t.i0 > k) break;
                const double wgt = (t.i0 == k ? (double)t.lam0 : 0.0) + (t.i1 == k ? (double)t.lam1 : 0.0);
                acc += wgt * (double)gb[n];
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) dmod[(size_t)b * dmod_stride + k] = (float)acc;
        }
    }
}

// C ABI ---------------------------------------------------------------------------------------
template <bool LR>
static int flanger_bwd_launch(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, const float *mod,
                              int64_t n_mod, const float *stash, const float *lfo_scale, const float *min_delay,
                              const float *feedback, const float *depth, const float *mix, const float *one_minus_mix,
                              const int32_t *max_delay, int32_t max_delay_max, const int32_t *rows, int64_t n_rows, int64_t B,
                              int64_t N, float *ws, float *dx, int64_t dx_stride, float *dmod, int64_t dmod_stride,
                              double *d_lfo_scale, double *d_min_delay, double *d_feedback, double *d_depth,
                              double *d_mix, void *stream)
{
    if (!dy || !x || !mod || !stash || !lfo_scale || !min_delay || !feedback || !depth || !mix || !one_minus_mix ||
        !max_delay || !ws || B <= 0 || N <= 0 || n_mod <= 0 || n_mod > N)
        return MX_ERR_ARG;
    if (max_delay_max < 2 || dy_stride < N || x_stride < N || (dx && dx_stride < N) || (dmod && dmod_stride < n_mod))
        return MX_ERR_ARG;
    if (max_delay_max > FL_MAX_M || max_delay_max > 65535 || N >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    const int64_t items = rows ? n_rows : B;
    if (items <= 0) return MX_OK;
    // LDS of the recurrence: A (max over the batch) + LR: the LFO row + the record ring (which holds float4 records)
    const int lfo_off = max_delay_max;
    const size_t lds_floats = ((size_t)max_delay_max + (LR ? (size_t)n_mod : 0) + 3) & ~(size_t)3;
    if (lds_floats > FL_MAX_M) return MX_ERR_UNSUPPORTED;
    const int ring_off = (int)lds_floats;
    static MxLdsLatch latch = {};                                       // one per instance of this template = per kernel
    if (mx_set_dyn_lds(latch, (const void *)fb_recur_kernel<LR>, (FL_MAX_M + FL_RING_FLOATS) * sizeof(float)) != MX_OK)
        return MX_ERR_LAUNCH;
    const size_t lds = (lds_floats + FL_RING_FLOATS) * sizeof(float);
    const float mod_scale = interp_scale_host(n_mod, N);
    hipLaunchKernelGGL(fb_recur_kernel<LR>, dim3((unsigned)items), dim3(FL_THREADS), lds, (hipStream_t)stream, dy,
                       (long long)dy_stride, x, (long long)x_stride, mod, stash, lfo_scale, min_delay, feedback, depth, mix,
                       one_minus_mix, max_delay, rows, (int)N, (int)n_mod, mod_scale, lfo_off, ring_off, ws);
    int rc = mx_launch_status();
    if (rc != MX_OK) return rc;
    hipLaunchKernelGGL(fb_out_kernel<LR>, dim3((unsigned)items), dim3(FB_OUT_THREADS), 0, (hipStream_t)stream, dy,
                       (long long)dy_stride, x, (long long)x_stride, mod, (int)n_mod, mod_scale, stash, ws, lfo_scale, min_delay,
                       feedback, depth, mix, one_minus_mix, max_delay, rows, (int)N, dx, (long long)dx_stride, dmod,
                       (long long)dmod_stride, d_lfo_scale, d_min_delay, d_feedback, d_depth, d_mix);
    return mx_launch_status();
}

MX_EXPORT int mx_flanger_bwd(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, const float *mod,
                             const float *stash, const float *lfo_scale, const float *min_delay, const float *feedback,
                             const float *depth, const float *mix, const float *one_minus_mix, const int32_t *max_delay,
                             int32_t max_delay_max, const int32_t *rows, int64_t n_rows, int64_t B, int64_t N,
                             float *ws, float *dx, int64_t dx_stride, float *dmod, int64_t dmod_stride,
                             double *d_lfo_scale, double *d_min_delay, double *d_feedback, double *d_depth,
                             double *d_mix, void *stream)
{
    return flanger_bwd_launch<false>(dy, dy_stride, x, x_stride, mod, N, stash, lfo_scale, min_delay, feedback, depth, mix,
                                     one_minus_mix, max_delay, max_delay_max, rows, n_rows, B, N, ws, dx, dx_stride, dmod,
                                     dmod_stride, d_lfo_scale, d_min_delay, d_feedback, d_depth, d_mix, stream);
}

// The adjoint for the LFO row the forward was given: mod (B, n_mod), 1 <= n_mod <= N, dmod (B, n_mod) with row stride
// dmod_stride >= n_mod.  n_mod == N is mx_flanger_bwd.
MX_EXPORT int mx_flanger_bwd_lr(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, const float *mod,
                                int64_t n_mod, const float *stash, const float *lfo_scale, const float *min_delay,
                                const float *feedback, const float *depth, const float *mix, const float *one_minus_mix,
                                const int32_t *max_delay, int32_t max_delay_max, const int32_t *rows, int64_t n_rows,
                                int64_t B, int64_t N, float *ws, float *dx, int64_t dx_stride, float *dmod,
                                int64_t dmod_stride, double *d_lfo_scale, double *d_min_delay, double *d_feedback,
                                double *d_depth, double *d_mix, void *stream)
{
    if (n_mod == N)
        return flanger_bwd_launch<false>(dy, dy_stride, x, x_stride, mod, N, stash, lfo_scale, min_delay, feedback, depth,
                                         mix, one_minus_mix, max_delay, max_delay_max, rows, n_rows, B, N, ws, dx, dx_stride,
                                         dmod, dmod_stride, d_lfo_scale, d_min_delay, d_feedback, d_depth, d_mix, stream);
    return flanger_bwd_launch<true>(dy, dy_stride, x, x_stride, mod, n_mod, stash, lfo_scale, min_delay, feedback, depth, mix,
                                    one_minus_mix, max_delay, max_delay_max, rows, n_rows, B, N, ws, dx, dx_stride, dmod,
                                    dmod_stride, d_lfo_scale, d_min_delay, d_feedback, d_depth, d_mix, stream);
}
