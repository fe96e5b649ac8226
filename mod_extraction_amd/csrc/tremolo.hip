// tremolo.hip -- K2c: tremolo (reference: mod_extraction/fx.py:13-22) and its adjoint.
//
// Memoryless: y[n] = (1 - mix) x[n] + (mix m[n]) x[n], one row per (clip, channel).  m is the LFO row itself (n_mod == N) or
// any shorter row resampled per sample with interp_tap / interp_combine (common.h) -- the pieces the flanger's fl_lfo is made
// of, with the scale of the same host helper -- so the low-rate path is bit-identical to
// apply_tremolo(x, linear_interpolate_last_dim(mod, N), mix).  The products round where the reference's separate torch ops
// round (explicit __f*_rn; the build has -ffp-contract=off).
//
// Forward: pure streaming, 8 B/sample with a low-rate LFO.  A workgroup owns a tile of TR_TILE samples of one row; rows whose
// pointers are 16-byte aligned move float4s, the ragged tail of a row and misaligned rows (channel 1 of a (B, 2, N) tensor
// with odd N) go one float at a time.
// Adjoint: one workgroup per row, no stash (m is recomputed as in the forward), no atomics, no (B, N) workspace:
//   pass 1  dx = dy (omm + mix m) in fp32, the fp64 partial sums of d mix = sum dy x (m - 1) (per thread, butterfly per wave,
//           the sixteen waves in order), and for n_mod == N dmod = mix dy x;
//   pass 2  (n_mod < N) one wave per low-rate point gathers the contiguous range of samples that have a tap on the point,
//           found the way flanger_bwd.hip finds it: weights are interp_tap's fp32 taps, products and sums fp64 in a fixed
//           order (per lane, then a butterfly), rounded once.  It re-reads dy and x, which pass 1 has just pulled through L2.
#include "common.h"

#define TR_THREADS 256
#define TR_TILE (TR_THREADS * 4 * 4)          // samples of one forward workgroup: four float4 per thread
#define TB_THREADS 1024
#define TB_WAVES (TB_THREADS / 64)

__device__ __forceinline__ float tr_mod(const float *__restrict__ row, float scale, int n, int n_mod, bool full)
{
    if (full) return row[n];
    const InterpTap t = interp_tap(scale, n, n_mod);
    return interp_combine(t, row[t.i0], row[t.i1]);
}
// fx.py:22, in the reference's order: ((1 - mix) * x) + ((mix * m) * x)
__device__ __forceinline__ float tr_y(float omm, float mx, float m, float x)
{
    return __fadd_rn(__fmul_rn(omm, x), __fmul_rn(__fmul_rn(mx, m), x));
}
__device__ __forceinline__ bool tr_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

__global__ __launch_bounds__(TR_THREADS) void tremolo_fwd_kernel(
    const float *__restrict__ x, long long x_stride, const float *__restrict__ mod, int n_mod, float mod_scale,
    const float *__restrict__ mix, const float *__restrict__ one_minus_mix, const int *__restrict__ rows, int N, int tiles,
    float *__restrict__ y, long long y_stride)
{
    const int item = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int b = rows ? rows[item] : item;
    const float mx = mix[b], omm = one_minus_mix[b];
    const float *xb = x + (size_t)b * x_stride;
    const float *mb = mod + (size_t)b * n_mod;
    float *yb = y + (size_t)b * y_stride;
    const bool full = n_mod == N;
    const int n0 = tile * TR_TILE;                                    // a multiple of 4
    const int n1 = min(N, n0 + TR_TILE);
    const bool vec = tr_aligned16(xb) && tr_aligned16(yb) && (!full || tr_aligned16(mb));
    const int nv = vec ? n0 + ((n1 - n0) & ~3) : n0;                  // [n0, nv) as float4, [nv, n1) one by one
    for (int n = n0 + 4 * (int)threadIdx.x; n < nv; n += 4 * TR_THREADS) {
        const float4 xv = *(const float4 *)(xb + n);
        float4 m;
        if (full) {
            m = *(const float4 *)(mb + n);
        } else {
            m.x = tr_mod(mb, mod_scale, n, n_mod, false);
            m.y = tr_mod(mb, mod_scale, n + 1, n_mod, false);
            m.z = tr_mod(mb, mod_scale, n + 2, n_mod, false);
            m.w = tr_mod(mb, mod_scale, n + 3, n_mod, false);
        }
        *(float4 *)(yb + n) = make_float4(tr_y(omm, mx, m.x, xv.x), tr_y(omm, mx, m.y, xv.y), tr_y(omm, mx, m.z, xv.z),
                                          tr_y(omm, mx, m.w, xv.w));
    }
    for (int n = nv + (int)threadIdx.x; n < n1; n += TR_THREADS)
        yb[n] = tr_y(omm, mx, tr_mod(mb, mod_scale, n, n_mod, full), xb[n]);
}

// one sample of pass 1; s accumulates d mix
__device__ __forceinline__ void tb_sample(float g, float xv, float m, float mx, float omm, float &dxv, float &dmv, double &s)
{
    const double p = (double)g * (double)xv;
    dxv = __fmul_rn(g, __fadd_rn(omm, __fmul_rn(mx, m)));
    dmv = (float)((double)mx * p);
    s += p * ((double)m - 1.0);
}

__global__ __launch_bounds__(TB_THREADS) void tremolo_bwd_kernel(
    const float *__restrict__ dy, long long dy_stride, const float *__restrict__ x, long long x_stride,
    const float *__restrict__ mod, int n_mod, float mod_scale, const float *__restrict__ mix,
    const float *__restrict__ one_minus_mix, const int *__restrict__ rows, int N, float *__restrict__ dx, long long dx_stride,
    float *__restrict__ dmod, double *__restrict__ dmix)
{
    __shared__ double red[TB_WAVES];
    const int b = rows ? rows[blockIdx.x] : (int)blockIdx.x;
    const float mx = mix[b], omm = one_minus_mix[b];
    const float *gb = dy + (size_t)b * dy_stride;
    const float *xb = x + (size_t)b * x_stride;
    const float *mb = mod + (size_t)b * n_mod;
    float *dxb = dx ? dx + (size_t)b * dx_stride : nullptr;
    float *dmb = dmod ? dmod + (size_t)b * n_mod : nullptr;
    const bool full = n_mod == N;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *dm_full = full ? dmb : nullptr;                            // n_mod == N: dmod is elementwise, written in pass 1

    if (dxb || dmix || dm_full) {
        double s = 0.0;
        const bool vec = tr_aligned16(gb) && tr_aligned16(xb) && (!dxb || tr_aligned16(dxb)) &&
                         (!full || (tr_aligned16(mb) && (!dm_full || tr_aligned16(dm_full))));
        const int nv = vec ? (N & ~3) : 0;
        for (int n = 4 * (int)threadIdx.x; n < nv; n += 4 * TB_THREADS) {
            const float4 g = *(const float4 *)(gb + n), xv = *(const float4 *)(xb + n);
            float4 m, o, d;
            if (full) {
                m = *(const float4 *)(mb + n);
            } else {
                m.x = tr_mod(mb, mod_scale, n, n_mod, false);
                m.y = tr_mod(mb, mod_scale, n + 1, n_mod, false);
                m.z = tr_mod(mb, mod_scale, n + 2, n_mod, false);
                m.w = tr_mod(mb, mod_scale, n + 3, n_mod, false);
            }
            tb_sample(g.x, xv.x, m.x, mx, omm, o.x, d.x, s);
            tb_sample(g.y, xv.y, m.y, mx, omm, o.y, d.y, s);
            tb_sample(g.z, xv.z, m.z, mx, omm, o.z, d.z, s);
            tb_sample(g.w, xv.w, m.w, mx, omm, o.w, d.w, s);
            if (dxb) *(float4 *)(dxb + n) = o;
            if (dm_full) *(float4 *)(dm_full + n) = d;
        }
        for (int n = nv + (int)threadIdx.x; n < N; n += TB_THREADS) {
            float o, d;
            tb_sample(gb[n], xb[n], tr_mod(mb, mod_scale, n, n_mod, full), mx, omm, o, d, s);
            if (dxb) dxb[n] = o;
            if (dm_full) dm_full[n] = d;
        }
        if (dmix) {
            s = wave_sum_f64(s);
            if (lane == 0) red[wv] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                double t = 0.0;
                for (int i = 0; i < TB_WAVES; ++i) t += red[i];
                dmix[b] = t;
            }
        }
    }
    if (dmb && !full) {
        for (int k = wv; k < n_mod; k += TB_WAVES) {
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
                acc += wgt * ((double)gb[n] * (double)xb[n]);
            }
            acc = wave_sum_f64(acc);
            if (lane == 0) dmb[k] = (float)((double)mx * acc);
        }
    }
}

// C ABI ---------------------------------------------------------------------------------------
// x: row b at x + b*x_stride (N samples); y likewise; mod (B,n_mod) dense with 1 <= n_mod <= N (n_mod < N: resampled
// in-kernel, align_corners=True); mix, one_minus_mix (B,) fp32; rows: optional list of n_rows row indices to process (others
// untouched).
MX_EXPORT int mx_tremolo_fwd(const float *x, int64_t x_stride, const float *mod, int64_t n_mod, const float *mix,
                             const float *one_minus_mix, const int32_t *rows, int64_t n_rows, int64_t B, int64_t N,
                             float *y, int64_t y_stride, void *stream)
{
    if (!x || !mod || !mix || !one_minus_mix || !y || B <= 0 || N <= 0 || n_mod <= 0 || n_mod > N) return MX_ERR_ARG;
    if (x_stride < N || y_stride < N || (rows && n_rows < 0)) return MX_ERR_ARG;
    if (N >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    const int64_t items = rows ? n_rows : B;
    if (items <= 0) return MX_OK;
    const int64_t tiles = (N + TR_TILE - 1) / TR_TILE;
    if (items * tiles >= (1ll << 31)) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tremolo_fwd_kernel, dim3((unsigned)(items * tiles)), dim3(TR_THREADS), 0, (hipStream_t)stream, x,
                       (long long)x_stride, mod, (int)n_mod, interp_scale_host(n_mod, N), mix, one_minus_mix, rows, (int)N,
                       (int)tiles, y, (long long)y_stride);
    return mx_launch_status();
}

// dy, x: views as in the forward; mod, n_mod, mix, one_minus_mix, rows: the forward's.  Optional outputs (NULL = skip):
// dx view (row stride dx_stride >= N), dmod (B,n_mod) fp32 dense, dmix (B,) fp64 (includes the one_minus_mix path).
MX_EXPORT int mx_tremolo_bwd(const float *dy, int64_t dy_stride, const float *x, int64_t x_stride, const float *mod,
                             int64_t n_mod, const float *mix, const float *one_minus_mix, const int32_t *rows,
                             int64_t n_rows, int64_t B, int64_t N, float *dx, int64_t dx_stride, float *dmod, double *dmix,
                             void *stream)
{
    if (!dy || !x || !mod || !mix || !one_minus_mix || B <= 0 || N <= 0 || n_mod <= 0 || n_mod > N) return MX_ERR_ARG;
    if (dy_stride < N || x_stride < N || (dx && dx_stride < N) || (rows && n_rows < 0)) return MX_ERR_ARG;
    if (N >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    const int64_t items = rows ? n_rows : B;
    if (items <= 0 || (!dx && !dmod && !dmix)) return MX_OK;
    if (items >= (1ll << 31)) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tremolo_bwd_kernel, dim3((unsigned)items), dim3(TB_THREADS), 0, (hipStream_t)stream, dy,
                       (long long)dy_stride, x, (long long)x_stride, mod, (int)n_mod, interp_scale_host(n_mod, N), mix,
                       one_minus_mix, rows, (int)N, dx, (long long)dx_stride, dmod, dmix);
    return mx_launch_status();
}
