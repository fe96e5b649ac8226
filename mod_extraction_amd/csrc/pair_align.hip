// pair_align.hip -- K19: the constant lag and the polarity of a recorded dry / wet pair by cross-correlation, and the integer
// shift that undoes them -- no counterpart in the reference (include/modex_hip.h, K19, has the definition).
//
//     r[b, l + L] = sum_n dry[b, n] wet[b, n + l]   (both indices in [0, N)),   l = -L..L
//     c = r / sqrt(sum dry^2 sum wet^2);  lag = argmax |c| (ties: smallest |l|, then l >= 0);  corr = c[lag];
//     frac = 0.5 (a - c+) / (a - 2 b0 + c+) on |c| at lag - 1, lag, lag + 1
//
// pair_xcorr_kernel  grid (tile of XC_LAGS = 64 lags, row), 256 threads.  The row is walked in tiles of XC_TN samples through
//     LDS, held there as fp64 (the conversion is done once a sample, not once a product): the dry tile, and the wet tile
//     widened by the 63 further samples the lag tile reaches, zeros outside the row.  Lane j of every wave owns lag l0 + j;
//     wave w takes quarter w of each time tile.  Per product one ds_read_b64 of wet at i + j (consecutive lanes: consecutive
//     banks), one of dry at i (one address: a broadcast) and one fp64 fma, whose product of two fp32 values is exact.  Fixed
//     order: a lane over time, then the four waves' partials 0 + 1 + 2 + 3 through LDS.  No atomics, no workspace.
//     LDS-issue bound: 4 clocks a wave-wide b64 read and CU against 1 for the fma; at 8 x 88200, L = 2205 that is 3.1 G
//     products on 552 workgroups.
// pair_peak_kernel   one 256-thread workgroup per row: the two energies (a thread strides the row, block256_sum_f64), then a
//     (|c|, l) arg-max under the tie rule -- a total order, so its result does not depend on the order of the reduction --
//     lanes by butterfly, the four waves through LDS; thread 0 forms frac in fp64 and rounds every output once.
// pair_shift_kernel  grid (chunks, row): out[b, n] = s_b wet[b, n + lag_b].  Chunk 0 is the scalar head up to the first
//     16-byte boundary of the out row, chunk q >= 1 four floats stored as one float4; the source is lag_b floats off that
//     alignment, so it is read through a 4-byte-aligned vector type.  Chunks at the row's tail or across the source's ends
//     go element by element with the bounds check.
#include "rows_common.h"

#define XC_THREADS 256
#define XC_WAVES (XC_THREADS / MX_WAVE)
#define XC_LAGS MX_WAVE
#define XC_TN 1024
#define XC_QUARTER (XC_TN / XC_WAVES)
#define PA_MAX_N (1ll << 24)
#define PA_MAX_L 8192
#define PA_MAX_B 65535

__global__ __launch_bounds__(XC_THREADS) void pair_xcorr_kernel(
    const float *__restrict__ dry, long long dry_stride, const float *__restrict__ wet, long long wet_stride, int N, int L,
    double *__restrict__ r_out)
{
    __shared__ double dry_s[XC_TN];
    __shared__ double wet_s[XC_TN + XC_LAGS];
    __shared__ double part[XC_WAVES][XC_LAGS];
    const int tid = (int)threadIdx.x, lane = tid & (MX_WAVE - 1), wave = tid / MX_WAVE;
    const size_t b = blockIdx.y;
    const int k0 = (int)blockIdx.x * XC_LAGS;                   // first column of this lag tile
    const int l0 = k0 - L;
    const float *d = dry + b * (size_t)dry_stride;
    const float *w = wet + b * (size_t)wet_stride;

    // the samples a lag of this tile pairs with something: dry index n in [max(0, -l), min(N, N - l)) over l in the tile
    const int l_hi = l0 + XC_LAGS - 1;
    const int n_lo = l_hi < 0 ? -l_hi : 0;
    const int n_hi = l0 > 0 ? N - l0 : N;

    double acc = 0.0;
    for (int n0 = n_lo; n0 < n_hi; n0 += XC_TN) {               // uniform over the workgroup
        __syncthreads();                                        // the tile before may still be read
        for (int i = tid; i < XC_TN; i += XC_THREADS) {
            const int n = n0 + i;
            dry_s[i] = n < N ? (double)d[n] : 0.0;              // n >= n_lo >= 0
        }
        for (int i = tid; i < XC_TN + XC_LAGS; i += XC_THREADS) {
            const long long m = (long long)n0 + l0 + i;
            wet_s[i] = (m >= 0 && m < N) ? (double)w[m] : 0.0;
        }
        __syncthreads();
        const double *dq = dry_s + wave * XC_QUARTER;
        const double *wq = wet_s + wave * XC_QUARTER + lane;    // i + lane <= XC_TN - 1 + 63
#pragma unroll 8
        for (int i = 0; i < XC_QUARTER; ++i) acc = fma(dq[i], wq[i], acc);
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && k0 + lane <= 2 * L)
        r_out[b * (size_t)(2 * L + 1) + k0 + lane] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

struct PeakBest { double a; int l; };                           // |c| and the lag it was found at

// the tie rule: larger |c|, then smaller |l|, then the non-negative lag
__device__ __forceinline__ bool peak_better(double a2, int l2, double a, int l)
{
    if (a2 != a) return a2 > a;
    const int m2 = l2 < 0 ? -l2 : l2, m = l < 0 ? -l : l;
    return m2 != m ? m2 < m : l2 > l;
}

__global__ __launch_bounds__(256) void pair_peak_kernel(
    const float *__restrict__ dry, long long dry_stride, const float *__restrict__ wet, long long wet_stride,
    const double *__restrict__ r, int N, int L, int *__restrict__ lag_out, float *__restrict__ corr_out,
    float *__restrict__ frac_out)
{
    __shared__ double red[4];
    __shared__ PeakBest best_s[4];
    const int tid = (int)threadIdx.x, lane = tid & (MX_WAVE - 1), wave = tid / MX_WAVE;
    const size_t b = blockIdx.x;
    const float *d = dry + b * (size_t)dry_stride;
    const float *w = wet + b * (size_t)wet_stride;
    const double *rr = r + b * (size_t)(2 * L + 1);

    double ed = 0.0, ew = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double x = (double)d[i], y = (double)w[i];
        ed = fma(x, x, ed);
        ew = fma(y, y, ew);
    }
    ed = block256_sum_f64(ed, red);
    ew = block256_sum_f64(ew, red);
    if (ed == 0.0 || ew == 0.0) {                               // uniform over the workgroup
        if (tid == 0) {
            lag_out[b] = 0;
            corr_out[b] = 0.0f;
            frac_out[b] = 0.0f;
        }
        return;
    }
    const double den = sqrt(ed * ew);

    PeakBest best;
    best.a = -1.0;
    best.l = 0;
    for (int k = tid; k <= 2 * L; k += 256) {
        const double a = fabs(rr[k] / den);
        if (peak_better(a, k - L, best.a, best.l)) {
            best.a = a;
            best.l = k - L;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a2 = __shfl_xor(best.a, o, MX_WAVE);
        const int l2 = __shfl_xor(best.l, o, MX_WAVE);
        if (peak_better(a2, l2, best.a, best.l)) {
            best.a = a2;
            best.l = l2;
        }
    }
    if (lane == 0) best_s[wave] = best;
    __syncthreads();
    if (tid != 0) return;
    best = best_s[0];
    for (int v = 1; v < 4; ++v)
        if (peak_better(best_s[v].a, best_s[v].l, best.a, best.l)) best = best_s[v];
    const int k = best.l + L;
    double frac = 0.0;
    if (k > 0 && k < 2 * L) {
        const double a = fabs(rr[k - 1] / den), c = fabs(rr[k + 1] / den);
        const double curv = (a - 2.0 * best.a) + c;
        if (curv != 0.0) frac = 0.5 * (a - c) / curv;
    }
    lag_out[b] = best.l;
    corr_out[b] = (float)(rr[k] / den);
    frac_out[b] = (float)frac;
}

__global__ __launch_bounds__(256) void pair_shift_kernel(
    const float *__restrict__ wet, long long wet_stride, int N, const int *__restrict__ lag, const float *__restrict__ corr,
    float *__restrict__ out, long long out_stride)
{
    const size_t b = blockIdx.y;
    const float *w = wet + b * (size_t)wet_stride;
    float *o = out + b * (size_t)out_stride;
    const long long sh = lag[b];
    const float s = (corr != nullptr && corr[b] < 0.0f) ? -1.0f : 1.0f;
    int head = rows_head(o);
    head = head < N ? head : N;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long start = q == 0 ? 0 : head + 4 * (q - 1);
    long long end = q == 0 ? head : start + 4;
    end = end < N ? end : N;
    if (start >= end) return;
    if (q > 0 && end - start == 4 && start + sh >= 0 && end + sh <= N) {
        const RowsUFloat4 v = *reinterpret_cast<const RowsUFloat4 *>(w + (start + sh));
        *reinterpret_cast<float4 *>(o + start) = make_float4(s * v.x, s * v.y, s * v.z, s * v.w);
        return;
    }
    for (long long n = start; n < end; ++n) {
        const long long m = n + sh;
        o[n] = (m >= 0 && m < N) ? s * w[m] : 0.0f;
    }
}

// C ABI ---------------------------------------------------------------------------------------
static int pair_check(const void *dry, int64_t dry_stride, const void *wet, int64_t wet_stride, int64_t B, int64_t N, int64_t L)
{
    if (!dry || !wet || B <= 0 || N <= 0 || L < 0 || L >= N || dry_stride < N || wet_stride < N) return MX_ERR_ARG;
    if (N > PA_MAX_N || L > PA_MAX_L || B > PA_MAX_B) return MX_ERR_UNSUPPORTED;
    return MX_OK;
}

MX_EXPORT int mx_pair_xcorr(const float *dry, int64_t dry_stride, const float *wet, int64_t wet_stride, int64_t B, int64_t N,
                            int64_t L, double *r_out, void *stream)
{
    if (!r_out) return MX_ERR_ARG;
    const int rc = pair_check(dry, dry_stride, wet, wet_stride, B, N, L);
    if (rc != MX_OK) return rc;
    const unsigned tiles = (unsigned)((2 * L + 1 + XC_LAGS - 1) / XC_LAGS);
    hipLaunchKernelGGL(pair_xcorr_kernel, dim3(tiles, (unsigned)B), dim3(XC_THREADS), 0, (hipStream_t)stream, dry,
                       (long long)dry_stride, wet, (long long)wet_stride, (int)N, (int)L, r_out);
    return mx_launch_status();
}

MX_EXPORT int mx_pair_peak(const float *dry, int64_t dry_stride, const float *wet, int64_t wet_stride, const double *r,
                           int64_t B, int64_t N, int64_t L, int32_t *lag_out, float *corr_out, float *frac_out, void *stream)
{
    if (!r || !lag_out || !corr_out || !frac_out) return MX_ERR_ARG;
    const int rc = pair_check(dry, dry_stride, wet, wet_stride, B, N, L);
    if (rc != MX_OK) return rc;
    hipLaunchKernelGGL(pair_peak_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, dry, (long long)dry_stride, wet,
                       (long long)wet_stride, r, (int)N, (int)L, lag_out, corr_out, frac_out);
    return mx_launch_status();
}

MX_EXPORT int mx_pair_shift(const float *wet, int64_t wet_stride, int64_t B, int64_t N, const int32_t *lag, const float *corr,
                            float *out, int64_t out_stride, void *stream)
{
    if (!lag || rows_check(wet, wet_stride, B, N) || rows_check(out, out_stride, B, N)) return MX_ERR_ARG;
    if (N > PA_MAX_N || B > PA_MAX_B) return MX_ERR_UNSUPPORTED;
    if (rows_overlap(rows_range(out, out_stride, B, N), rows_range(wet, wet_stride, B, N))) return MX_ERR_ARG;   // no aliasing
    const long long chunks = 1 + (N + 3) / 4;                   // the head, then float4s: covers every head length 0..3
    hipLaunchKernelGGL(pair_shift_kernel, dim3((unsigned)((chunks + 255) / 256), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, wet, (long long)wet_stride, (int)N, (const int *)lag, corr, out,
                       (long long)out_stride);
    return mx_launch_status();
}
