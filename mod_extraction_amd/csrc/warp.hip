// warp.hip -- K26: rows of fp32 audio read along a straight line of fractional positions (warp_abi.h has the definition) --
// no counterpart in the reference.  A wet recorded on another clock than its dry is put on the dry's time base with it.
//
// warp_rows_kernel   grid (output tile, row), WP_THREADS threads, MX_WARP_OUT_TILE outputs of one row a workgroup: thread t
//     computes the outputs t, t + WP_THREADS, ... of the tile, one output a lane a pass.  pos(m) is non-decreasing in m
//     (each of its three roundings is monotone), so the tile reads x[floor(pos(first)) - half .. floor(pos(last)) + half]:
//     at most WP_TILE_SPAN + T + 2 samples, staged once in LDS behind an index test (0 outside the row).  The taps depend
//     on f, which differs from output to output, so there is no shared polyphase table; what the outputs share is
//       cs   (cos, sin)(pi c j), j = -half .. half, fp64: sin(pi c (f + j)) by angle addition from one sincos(pi c f) an
//            output.  Its absolute error is that of sin at an argument of up to pi c half, which the division by pi c tau
//            then scales: harmless for |tau| >= 1 and not below, so the two taps with |tau| < 1 call sin;
//       inv  1 / j^2, j < WP_I0_TERMS, fp64: the I0 series multiplies where K24's divides.  beta <= 64 ends the series
//            before j = 90, so the table's length never binds and the stopping rule is K24's.
//     A tap is c sinc(c tau) I0(..) (1 / I0(beta)), 1 / I0(beta) from the host.  The sum is fma(h, (double)x, acc) in
//     ascending k over the taps whose sample lies in the row, one rounding at the store.  No atomics, no workspace, every
//     output written by exactly one thread.  A row whose drift or offset is beyond the limits (they are device words) is
//     written as NaNs by the same grid.
#include "rows_common.h"
#include "warp_abi.h"

#define WP_THREADS 256
#define WP_I0_TERMS 256
#define WP_TILE_SPAN 1026                                       // ceil(MX_WARP_OUT_TILE (1 + MX_WARP_MAX_DRIFT))

static_assert(MX_WARP_OUT_TILE % WP_THREADS == 0, "a tile is a whole number of passes of the workgroup");
static_assert((double)WP_TILE_SPAN >= MX_WARP_OUT_TILE * (1.0 + MX_WARP_MAX_DRIFT) && WP_TILE_SPAN - 1 < MX_WARP_OUT_TILE * (1.0 + MX_WARP_MAX_DRIFT),
              "WP_TILE_SPAN is the ceiling of a tile's reach at the largest drift");

// bytes of LDS for T taps: cs (2 T doubles), inv (WP_I0_TERMS doubles), the staged samples (WP_TILE_SPAN + T + 2 floats)
static inline size_t wp_lds_bytes(int64_t T)
{
    return (size_t)(8 * (2 * T + WP_I0_TERMS) + 4 * (WP_TILE_SPAN + T + 2));
}
static_assert(8 * (2 * MX_WARP_MAX_TAPS + WP_I0_TERMS) + 4 * (WP_TILE_SPAN + MX_WARP_MAX_TAPS + 2) <= 160 * 1024, "the LDS of one CU");

// I0 by its power series in ascending j, until a term falls below 2^-60 of the sum; inv[j] = 1 / j^2
__device__ __forceinline__ double wp_i0(double x, const double *inv)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int j = 1; j < WP_I0_TERMS; ++j) {
        term = term * q * inv[j];
        sum += term;
        if (term < sum * 0x1p-60) break;
    }
    return sum;
}

// pos = m + (m drift + offset), three roundings
__device__ __forceinline__ double wp_pos(long long m, double drift, double offset)
{
    const double md = (double)m;
    return __dadd_rn(md, __dadd_rn(__dmul_rn(md, drift), offset));
}

__global__ __launch_bounds__(WP_THREADS) void warp_rows_kernel(const float *__restrict__ x, long long x_stride, long long b0,
                                                               long long n_in, const double *__restrict__ offset,
                                                               const double *__restrict__ drift, const float *__restrict__ sign,
                                                               int half, double c, double beta, double inv_i0b,
                                                               float *__restrict__ y, long long y_stride, long long n_out)
{
    extern __shared__ double wp_lds[];
    const int tid = (int)threadIdx.x;
    const int T = 2 * half + 1;
    double *cs = wp_lds;                                        // (cos, sin)(pi c (t - half)) at 2 t, 2 t + 1
    double *inv = cs + 2 * T;
    float *xs = (float *)(inv + WP_I0_TERMS);
    const int cap = WP_TILE_SPAN + T + 2;

    const size_t b = (size_t)b0 + blockIdx.y;
    const float *xr = x + b * (size_t)x_stride;
    float *yr = y + b * (size_t)y_stride;
    const double off = offset[b], dr = drift[b];
    const double s = (sign && sign[b] < 0.0f) ? -1.0 : 1.0;
    const long long m_first = (long long)blockIdx.x * MX_WARP_OUT_TILE;
    const long long m_end = m_first + MX_WARP_OUT_TILE < n_out ? m_first + MX_WARP_OUT_TILE : n_out;       // > m_first

    // the same words in every thread: the branch is uniform over the workgroup
    bool ok = fabs(dr) <= MX_WARP_MAX_DRIFT && fabs(off) < MX_WARP_MAX_OFFSET;                             // false for NaN
    long long i_first = 0;
    int count = 0;
    if (ok) {
        i_first = (long long)floor(wp_pos(m_first, dr, off)) - half;
        const long long n = (long long)floor(wp_pos(m_end - 1, dr, off)) + half - i_first + 1;
        ok = n >= 1 && n <= cap;                                // holds by the bound above; the staging relies on it
        count = (int)n;
    }
    if (!ok) {
        for (long long m = m_first + tid; m < m_end; m += WP_THREADS) yr[m] = __int_as_float(0x7FC00000);
        return;
    }
    for (int t = tid; t < T; t += WP_THREADS) {
        double sn, cn;
        sincos(M_PI * (c * (double)(t - half)), &sn, &cn);
        cs[2 * t] = cn;
        cs[2 * t + 1] = sn;
    }
    for (int j = tid; j < WP_I0_TERMS; j += WP_THREADS) inv[j] = j ? 1.0 / ((double)j * (double)j) : 0.0;
    for (int i = tid; i < count; i += WP_THREADS) {
        const long long g = i_first + i;
        xs[i] = (g >= 0 && g < n_in) ? xr[g] : 0.0f;
    }
    __syncthreads();

    const double dhalf = (double)half;
    for (long long m = m_first + tid; m < m_end; m += WP_THREADS) {
        const double pos = wp_pos(m, dr, off), fl = floor(pos), f = pos - fl;
        const long long i0 = (long long)fl;
        long long lo = (long long)half - i0, hi = n_in + half - i0;       // the taps k in lo .. hi - 1 meet the row
        lo = lo < 0 ? 0 : (lo > T ? T : lo);
        hi = hi < 0 ? 0 : (hi > T ? T : hi);
        const int base = (int)(i0 - half - i_first);            // 0 <= base, base + T - 1 < count
        double sf, cf;
        sincos(M_PI * (c * f), &sf, &cf);
        double acc = 0.0;
        for (int k = (int)lo; k < (int)hi; ++k) {
            const int j = half - k;
            const double tau = f + (double)j;
            if (tau > dhalf) continue;                          // k = 0 with f > 0: beyond the window (tau >= -half always)
            const double xc = c * tau, pix = M_PI * xc;
            const double sn = fabs(tau) < 1.0 ? sin(pix) : sf * cs[2 * (j + half)] + cf * cs[2 * (j + half) + 1];
            const double sc = xc == 0.0 ? 1.0 : sn / pix;
            const double r = tau / dhalf;
            const double w = wp_i0(beta * sqrt(fmax(0.0, 1.0 - r * r)), inv);
            acc = fma(c * sc * w * inv_i0b, (double)xs[base + k], acc);
        }
        yr[m] = (float)(s * acc);
    }
}

// C ABI (warp_abi.h) ---------------------------------------------------------------------------
static double wp_host_i0(double x)                              // K24's series as it stands, on the host
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int j = 1; j < 1000; ++j) {
        term = term * q / ((double)j * (double)j);
        sum += term;
        if (term < sum * 0x1p-60) break;
    }
    return sum;
}

static inline bool wp_filter_ok(int32_t zeros, double rolloff, double beta)
{
    return zeros >= 1 && rolloff > 0.0 && rolloff <= 1.0 && beta >= 0.0;
}

// half and the number of tiles, or the limit that refuses them
static int wp_limits(int32_t zeros, double rolloff, double beta, int64_t n_in, int64_t n_out, int64_t &half, int64_t &tiles)
{
    if (beta > MX_WARP_MAX_BETA) return MX_ERR_UNSUPPORTED;
    const double hf = ceil((double)zeros / rolloff);
    if (!(2.0 * hf + 1.0 <= (double)MX_WARP_MAX_TAPS)) return MX_ERR_UNSUPPORTED;
    if (n_in > MX_WARP_MAX_N || n_out > MX_WARP_MAX_N) return MX_ERR_UNSUPPORTED;
    half = (int64_t)hf;
    tiles = (n_out + MX_WARP_OUT_TILE - 1) / MX_WARP_OUT_TILE;
    return tiles > 2147483647LL ? MX_ERR_UNSUPPORTED : MX_OK;
}

MX_EXPORT int mx_warp_plan(int32_t zeros, double rolloff, double beta, int64_t n_in, int64_t n_out, double drift_bound,
                           double offset_bound, int32_t *half, int32_t *taps, int64_t *tiles, int32_t *span)
{
    if (!half || !taps || !tiles || !span) return MX_ERR_ARG;
    if (!wp_filter_ok(zeros, rolloff, beta) || n_in < 1 || n_out < 1 || !(drift_bound >= 0.0) || !(offset_bound >= 0.0))
        return MX_ERR_ARG;
    int64_t h, nt;
    const int rc = wp_limits(zeros, rolloff, beta, n_in, n_out, h, nt);
    if (rc != MX_OK) return rc;
    if (drift_bound > MX_WARP_MAX_DRIFT || offset_bound >= MX_WARP_MAX_OFFSET) return MX_ERR_UNSUPPORTED;
    *half = (int32_t)h;
    *taps = (int32_t)(2 * h + 1);
    *tiles = nt;
    *span = (int32_t)(WP_TILE_SPAN + 2 * h + 1 + 2);
    return MX_OK;
}

MX_EXPORT int mx_warp_rows(const float *x, int64_t x_stride, int64_t B, int64_t n_in, const double *offset, const double *drift,
                           const float *sign, int32_t zeros, double rolloff, double beta, float *y, int64_t y_stride,
                           int64_t n_out, void *stream)
{
    static MxLdsLatch latch;
    if (!offset || !drift || rows_check(x, x_stride, B, n_in) != MX_OK || rows_check(y, y_stride, B, n_out) != MX_OK)
        return MX_ERR_ARG;
    if (!wp_filter_ok(zeros, rolloff, beta)) return MX_ERR_ARG;
    int64_t half, tiles;
    int rc = wp_limits(zeros, rolloff, beta, n_in, n_out, half, tiles);
    if (rc != MX_OK) return rc;
    const RowsRange out = rows_range(y, y_stride, B, n_out);
    const RowsRange in[4] = {rows_range(x, x_stride, B, n_in), rows_flat(offset, B, 8), rows_flat(drift, B, 8),
                             rows_flat(sign, sign ? B : 0, 4)};
    if (rows_any_overlap(&out, 1, in, 4)) return MX_ERR_ARG;
    rc = mx_set_dyn_lds(latch, (const void *)warp_rows_kernel, wp_lds_bytes(MX_WARP_MAX_TAPS));
    if (rc != MX_OK) return rc;
    const double inv_i0b = 1.0 / wp_host_i0(beta);
    hipStream_t st = (hipStream_t)stream;
    for (int64_t b0 = 0; b0 < B; b0 += MX_WARP_MAX_ROWS) {
        const unsigned rows = (unsigned)(B - b0 < MX_WARP_MAX_ROWS ? B - b0 : MX_WARP_MAX_ROWS);
        hipLaunchKernelGGL(warp_rows_kernel, dim3((unsigned)tiles, rows), dim3(WP_THREADS), wp_lds_bytes(2 * half + 1), st, x,
                           (long long)x_stride, (long long)b0, (long long)n_in, offset, drift, sign, (int)half, rolloff, beta,
                           inv_i0b, y, (long long)y_stride, (long long)n_out);
    }
    return mx_launch_status();
}
