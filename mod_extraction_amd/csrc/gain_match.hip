// gain_match.hip -- K20: one gain per clip that carries a rendered wet (y_hat) onto a recorded one (y), forward and
// backward -- no counterpart in the reference (include/modex_hip.h, K20, has the definition).
//
//     a = <y_hat, y_hat>, c = <y_hat, y>, e = <y, y>;   "ls": g = c / (a + eps);   "rms": g = sqrt((e + eps) / (a + eps))
//     z = fl32(fl32(g) * y_hat);   s = <dz, y_hat>;   dy_hat = g dz + s dg/dy_hat  (a clamped row: g dz)
//
// All four kernels: grid (chunk, row), 256 threads, a workgroup owns GM_CHUNK = 2048 samples of one row.  A chunk is walked as
// a scalar head up to the first 16-byte boundary of its LEADING array (0..3 floats), float4s, and a scalar tail (0..3 floats).
// GM_CHUNK is a multiple of 4, so every chunk of a row has the row's head.  The leading array -- the one that is stored
// where there is one (z, dy_hat), else y_hat -- is accessed as aligned float4 (global_load/store_dwordx4, a wave covers
// 1 KiB contiguously); the other arrays of the same elements may sit at another offset from a 16-byte boundary and are read
// through a 4-byte-aligned vector type, which is still one dwordx4 load.  So a row may start anywhere.
//
// gain_partials_kernel      a thread accumulates its products in fp64 (fma on two converted fp32 values: the product is
//     exact) in the order head, float4s, tail; the workgroup's three sums (lanes by butterfly, the four waves 0 + 1 + 2 + 3
//     through LDS) go to partials[b, chunk, 0:3].
// gain_apply_kernel         every workgroup re-reduces its row's n_chunks partials (thread t takes chunks t, t + 256, ..; the
//     same block sum), so all of a row's workgroups hold the same a, c, e and the same g without a third launch; chunk 0
//     writes gain, sums, flags.  z = __fmul_rn(g, y_hat).
// gain_bwd_partials_kernel  the partial <dz, y_hat> of the chunk, likewise.
// gain_bwd_apply_kernel     re-reduces s, k = s / (a + eps) once a workgroup, then per element in fp64
//     "ls": fma(g, dz, k (y - 2 g y_hat)),  "rms": fma(g, dz, -(k g) y_hat),  clamped: g dz -- rounded once.  A thread reads
//     dz[i] before it writes dy_hat[i] and nobody else touches i, so dy_hat may be dz.
// Memory bound: forward 2 reads + (1 read, 1 write) of B N floats, backward 2 + (3, 1).
#include "rows_common.h"

#define GM_THREADS 256
#define GM_CHUNK MX_GAIN_CHUNK
#define GM_MAX_N (1ll << 24)
#define GM_MAX_B 65535

static_assert(GM_CHUNK % 4 == 0, "every chunk of a row shares the row's head");

// three block sums at once; red: 12 doubles of LDS.  Fixed order: lanes by butterfly, then waves 0 + 1 + 2 + 3.
__device__ __forceinline__ void gm_block_sum3(double &a, double &c, double &e, double *red)
{
    a = wave_sum_f64(a);
    c = wave_sum_f64(c);
    e = wave_sum_f64(e);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[w] = a;
        red[4 + w] = c;
        red[8 + w] = e;
    }
    __syncthreads();
    a = ((red[0] + red[1]) + red[2]) + red[3];
    c = ((red[4] + red[5]) + red[6]) + red[7];
    e = ((red[8] + red[9]) + red[10]) + red[11];
}

__global__ __launch_bounds__(GM_THREADS) void gain_partials_kernel(
    const float *__restrict__ y_hat, long long y_hat_stride, const float *__restrict__ y, long long y_stride, int N,
    double *__restrict__ partials)
{
    __shared__ double red[12];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * GM_CHUNK;
    const int len = min(GM_CHUNK, N - n0);                          // >= 1: the grid has ceil(N / GM_CHUNK) chunks
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    const float *q = y + b * (size_t)y_stride + n0;
    const RowsSpan sp = rows_span(p, len);
    double a = 0.0, c = 0.0, e = 0.0;
    if (tid < sp.head) {
        const double u = (double)p[tid], v = (double)q[tid];
        a = fma(u, u, a);
        c = fma(u, v, c);
        e = fma(v, v, e);
    }
    const float4 *pv = reinterpret_cast<const float4 *>(p + sp.head);
    const RowsUFloat4 *qv = reinterpret_cast<const RowsUFloat4 *>(q + sp.head);
    for (int i = tid; i < sp.nvec; i += GM_THREADS) {
        const float4 u4 = pv[i];
        const RowsUFloat4 v4 = qv[i];
        const double u[4] = {(double)u4.x, (double)u4.y, (double)u4.z, (double)u4.w};
        const double v[4] = {(double)v4.x, (double)v4.y, (double)v4.z, (double)v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a = fma(u[j], u[j], a);
            c = fma(u[j], v[j], c);
            e = fma(v[j], v[j], e);
        }
    }
    if (tid < sp.tail) {
        const int i = sp.head + 4 * sp.nvec + tid;
        const double u = (double)p[i], v = (double)q[i];
        a = fma(u, u, a);
        c = fma(u, v, c);
        e = fma(v, v, e);
    }
    gm_block_sum3(a, c, e, red);
    if (tid == 0) {
        double *o = partials + (b * gridDim.x + blockIdx.x) * 3;
        o[0] = a;
        o[1] = c;
        o[2] = e;
    }
}

__global__ __launch_bounds__(GM_THREADS) void gain_apply_kernel(
    const float *__restrict__ y_hat, long long y_hat_stride, const double *__restrict__ partials, int N, int mode, double eps,
    int clamp, double lo, double hi, float *__restrict__ z, long long z_stride, float *__restrict__ gain,
    double *__restrict__ sums, int *__restrict__ flags)
{
    __shared__ double red[12];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const int n_chunks = (int)gridDim.x;
    const double *pr = partials + b * (size_t)n_chunks * 3;
    double a = 0.0, c = 0.0, e = 0.0;
    for (int k = tid; k < n_chunks; k += GM_THREADS) {
        a += pr[3 * k];
        c += pr[3 * k + 1];
        e += pr[3 * k + 2];
    }
    gm_block_sum3(a, c, e, red);
    double g64 = mode == MX_GAIN_LS ? c / (a + eps) : sqrt((e + eps) / (a + eps));
    int flag = 0;
    if (clamp) {
        if (g64 < lo) { g64 = lo; flag = 1; }
        if (g64 > hi) { g64 = hi; flag = 1; }
    }
    const float g = (float)g64;
    if (blockIdx.x == 0 && tid == 0) {
        gain[b] = g;
        sums[3 * b] = a;
        sums[3 * b + 1] = c;
        sums[3 * b + 2] = e;
        flags[b] = flag;
    }
    const int n0 = (int)blockIdx.x * GM_CHUNK;
    const int len = min(GM_CHUNK, N - n0);
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    float *o = z + b * (size_t)z_stride + n0;
    const RowsSpan sp = rows_span(o, len);
    if (tid < sp.head) o[tid] = __fmul_rn(g, p[tid]);
    const RowsUFloat4 *pv = reinterpret_cast<const RowsUFloat4 *>(p + sp.head);
    float4 *ov = reinterpret_cast<float4 *>(o + sp.head);
    for (int i = tid; i < sp.nvec; i += GM_THREADS) {
        const RowsUFloat4 u = pv[i];
        ov[i] = make_float4(__fmul_rn(g, u.x), __fmul_rn(g, u.y), __fmul_rn(g, u.z), __fmul_rn(g, u.w));
    }
    if (tid < sp.tail) {
        const int i = sp.head + 4 * sp.nvec + tid;
        o[i] = __fmul_rn(g, p[i]);
    }
}

__global__ __launch_bounds__(GM_THREADS) void gain_bwd_partials_kernel(
    const float *__restrict__ dz, long long dz_stride, const float *__restrict__ y_hat, long long y_hat_stride, int N,
    double *__restrict__ partials)
{
    __shared__ double red[4];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * GM_CHUNK;
    const int len = min(GM_CHUNK, N - n0);
    const float *p = dz + b * (size_t)dz_stride + n0;
    const float *q = y_hat + b * (size_t)y_hat_stride + n0;
    const RowsSpan sp = rows_span(p, len);
    double s = 0.0;
    if (tid < sp.head) s = fma((double)p[tid], (double)q[tid], s);
    const float4 *pv = reinterpret_cast<const float4 *>(p + sp.head);
    const RowsUFloat4 *qv = reinterpret_cast<const RowsUFloat4 *>(q + sp.head);
    for (int i = tid; i < sp.nvec; i += GM_THREADS) {
        const float4 u = pv[i];
        const RowsUFloat4 v = qv[i];
        s = fma((double)u.x, (double)v.x, s);
        s = fma((double)u.y, (double)v.y, s);
        s = fma((double)u.z, (double)v.z, s);
        s = fma((double)u.w, (double)v.w, s);
    }
    if (tid < sp.tail) {
        const int i = sp.head + 4 * sp.nvec + tid;
        s = fma((double)p[i], (double)q[i], s);
    }
    s = block256_sum_f64(s, red);
    if (tid == 0) partials[b * gridDim.x + blockIdx.x] = s;
}

// one element of the backward in fp64, rounded once; k = s / (a + eps), kg = k g (both 0 on a clamped row)
__device__ __forceinline__ float gm_bwd_one(int mode, double g, double k, double kg, float dz, float yh, float y)
{
    if (mode == MX_GAIN_LS) return (float)fma(g, (double)dz, k * fma(-2.0 * g, (double)yh, (double)y));
    return (float)fma(g, (double)dz, -(kg * (double)yh));
}

__global__ __launch_bounds__(GM_THREADS) void gain_bwd_apply_kernel(
    const float *dz, long long dz_stride, const float *__restrict__ y_hat, long long y_hat_stride,
    const float *__restrict__ y, long long y_stride, const float *__restrict__ gain, const double *__restrict__ sums,
    const int *__restrict__ flags, const double *__restrict__ partials, int N, int mode, double eps, float *dy_hat,
    long long dy_hat_stride)
{
    __shared__ double red[4];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const int n_chunks = (int)gridDim.x;
    const double *pr = partials + b * (size_t)n_chunks;
    double s = 0.0;
    for (int k = tid; k < n_chunks; k += GM_THREADS) s += pr[k];
    s = block256_sum_f64(s, red);
    const double g = (double)gain[b];
    const double k = flags[b] ? 0.0 : s / (sums[3 * b] + eps);
    const double kg = k * g;
    const int n0 = (int)blockIdx.x * GM_CHUNK;
    const int len = min(GM_CHUNK, N - n0);
    const float *d = dz + b * (size_t)dz_stride + n0;
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    const float *q = y + b * (size_t)y_stride + n0;
    float *o = dy_hat + b * (size_t)dy_hat_stride + n0;
    const RowsSpan sp = rows_span(o, len);
    if (tid < sp.head) o[tid] = gm_bwd_one(mode, g, k, kg, d[tid], p[tid], q[tid]);
    const RowsUFloat4 *dv = reinterpret_cast<const RowsUFloat4 *>(d + sp.head);
    const RowsUFloat4 *pv = reinterpret_cast<const RowsUFloat4 *>(p + sp.head);
    const RowsUFloat4 *qv = reinterpret_cast<const RowsUFloat4 *>(q + sp.head);
    float4 *ov = reinterpret_cast<float4 *>(o + sp.head);
    for (int i = tid; i < sp.nvec; i += GM_THREADS) {
        const RowsUFloat4 u = dv[i], v = pv[i], w = qv[i];
        ov[i] = make_float4(gm_bwd_one(mode, g, k, kg, u.x, v.x, w.x), gm_bwd_one(mode, g, k, kg, u.y, v.y, w.y),
                            gm_bwd_one(mode, g, k, kg, u.z, v.z, w.z), gm_bwd_one(mode, g, k, kg, u.w, v.w, w.w));
    }
    if (tid < sp.tail) {
        const int i = sp.head + 4 * sp.nvec + tid;
        o[i] = gm_bwd_one(mode, g, k, kg, d[i], p[i], q[i]);
    }
}

// C ABI ---------------------------------------------------------------------------------------
static int gm_check_size(int64_t B, int64_t N)
{
    return (N > GM_MAX_N || B > GM_MAX_B) ? MX_ERR_UNSUPPORTED : MX_OK;
}

static dim3 gm_grid(int64_t B, int64_t N)
{
    return dim3((unsigned)((N + GM_CHUNK - 1) / GM_CHUNK), (unsigned)B);
}

MX_EXPORT int mx_gain_match_partials(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                                     int64_t N, double *partials, void *stream)
{
    if (!partials || rows_check(y_hat, y_hat_stride, B, N) || rows_check(y, y_stride, B, N)) return MX_ERR_ARG;
    if (gm_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gain_partials_kernel, gm_grid(B, N), dim3(GM_THREADS), 0, (hipStream_t)stream, y_hat,
                       (long long)y_hat_stride, y, (long long)y_stride, (int)N, partials);
    return mx_launch_status();
}

static bool gm_bad_mode_eps(int32_t mode, double eps)
{
    return (mode != MX_GAIN_LS && mode != MX_GAIN_RMS) || !(eps > 0.0) || !(eps < 1e300);
}

MX_EXPORT int mx_gain_match_apply(const float *y_hat, int64_t y_hat_stride, const double *partials, int64_t B, int64_t N,
                                  int32_t mode, double eps, int32_t clamp, double lo, double hi, float *z, int64_t z_stride,
                                  float *gain, double *sums, int32_t *flags, void *stream)
{
    if (!partials || !gain || !sums || !flags || rows_check(y_hat, y_hat_stride, B, N) || rows_check(z, z_stride, B, N))
        return MX_ERR_ARG;
    if (gm_bad_mode_eps(mode, eps)) return MX_ERR_ARG;
    if (clamp && !(0.0 < lo && lo <= 1.0 && 1.0 <= hi && hi < 1e300)) return MX_ERR_ARG;
    if (gm_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    if (rows_overlap(rows_range(z, z_stride, B, N), rows_range(y_hat, y_hat_stride, B, N))) return MX_ERR_ARG;
    hipLaunchKernelGGL(gain_apply_kernel, gm_grid(B, N), dim3(GM_THREADS), 0, (hipStream_t)stream, y_hat,
                       (long long)y_hat_stride, partials, (int)N, (int)mode, eps, (int)clamp, lo, hi, z, (long long)z_stride,
                       gain, sums, (int *)flags);
    return mx_launch_status();
}

MX_EXPORT int mx_gain_match_bwd_partials(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride,
                                         int64_t B, int64_t N, double *partials, void *stream)
{
    if (!partials || rows_check(dz, dz_stride, B, N) || rows_check(y_hat, y_hat_stride, B, N)) return MX_ERR_ARG;
    if (gm_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gain_bwd_partials_kernel, gm_grid(B, N), dim3(GM_THREADS), 0, (hipStream_t)stream, dz,
                       (long long)dz_stride, y_hat, (long long)y_hat_stride, (int)N, partials);
    return mx_launch_status();
}

MX_EXPORT int mx_gain_match_bwd_apply(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride,
                                      const float *y, int64_t y_stride, const float *gain, const double *sums,
                                      const int32_t *flags, const double *partials, int64_t B, int64_t N, int32_t mode,
                                      double eps, float *dy_hat, int64_t dy_hat_stride, void *stream)
{
    if (!gain || !sums || !flags || !partials || rows_check(dz, dz_stride, B, N) || rows_check(y_hat, y_hat_stride, B, N)
        || rows_check(y, y_stride, B, N) || rows_check(dy_hat, dy_hat_stride, B, N))
        return MX_ERR_ARG;
    if (gm_bad_mode_eps(mode, eps)) return MX_ERR_ARG;
    if (gm_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    const bool in_place = dy_hat == dz && dy_hat_stride == dz_stride;
    const RowsRange out = rows_range(dy_hat, dy_hat_stride, B, N);
    if ((!in_place && rows_overlap(out, rows_range(dz, dz_stride, B, N)))
        || rows_overlap(out, rows_range(y_hat, y_hat_stride, B, N)) || rows_overlap(out, rows_range(y, y_stride, B, N)))
        return MX_ERR_ARG;
    hipLaunchKernelGGL(gain_bwd_apply_kernel, gm_grid(B, N), dim3(GM_THREADS), 0, (hipStream_t)stream, dz,
                       (long long)dz_stride, y_hat, (long long)y_hat_stride, y, (long long)y_stride, gain, sums,
                       (const int *)flags, partials, (int)N, (int)mode, eps, dy_hat, (long long)dy_hat_stride);
    return mx_launch_status();
}
