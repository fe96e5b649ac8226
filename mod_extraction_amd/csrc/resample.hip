// resample.hip -- K24: band-limited rational sample-rate conversion of rows of fp32 audio (resample_abi.h has the
// definition) -- no counterpart in the reference, which drops every file that is not at the training rate.
//
// resample_taps_kernel   one thread per table entry, all of it in fp64, one rounding to fp32.
// resample_rows_kernel   grid (output tile, row), RS_THREADS threads, MX_RESAMPLE_OUT_TILE outputs of one row a workgroup:
//     thread t computes the outputs t, t + RS_THREADS, ... of the tile, so the lanes of a wave hold consecutive outputs --
//     their input windows x[i0 - half .. i0 + half] start down / up samples apart, and a step of k is one coalesced read of
//     about 64 down / up consecutive floats that L1 serves after the first touch; x is not staged.  Two instantiations:
//       LDS  the whole (up, T) table is copied to LDS once a workgroup (65 KB for 48 -> 44.1 kHz, 130 KB for 96 -> 44.1 kHz:
//            one workgroup a CU, which is why it has 16 waves).  256 consecutive outputs already touch every phase, so a
//            small tile would pay more for the copy than for its arithmetic; over 4096 outputs the copy is up T / 4096 =
//            4 .. 8 floats an output against T = 111 .. 221 FMAs.  A phase is a row of T floats, T odd: lane l reads word
//            p_l T + k, and the phases of consecutive outputs differ (gcd(up, down) = 1), so conflicts are the chance
//            coincidences of p_l T mod 32 and not a systematic stride.
//       L2   the table does not fit (44.1 -> 32 kHz: 320 x 141 floats = 180 KB): taps[p][k] is read from global memory; the
//            table is shared by every workgroup and stays in L2, a lane walks its row of T floats in ascending k.
//     The sum is the definition's: (double)tap * (double)x is exact, fma adds it to the fp64 accumulator in ascending k,
//     one rounding at the store.  No atomics, no workspace, every output written by exactly one thread.
#include "rows_common.h"
#include "resample_abi.h"

#define RS_THREADS 1024
#define RS_PER_THREAD (MX_RESAMPLE_OUT_TILE / RS_THREADS)
#define RS_MAX_ROWS 65535                                       // grid.y of a launch
#define RS_TAPS_THREADS 256

static_assert(MX_RESAMPLE_OUT_TILE % RS_THREADS == 0, "a tile is a whole number of passes of the workgroup");
static_assert(MX_RESAMPLE_LDS_TABLE_BYTES <= 160 * 1024, "the LDS of one CU");

// I0 by its power series in ascending j, until a term falls below 2^-60 of the sum
__device__ __forceinline__ double rs_i0(double x)
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

__global__ __launch_bounds__(RS_TAPS_THREADS) void resample_taps_kernel(int up, int half, double c, double beta,
                                                                        float *__restrict__ taps)
{
    const int T = 2 * half + 1;
    const int e = (int)(blockIdx.x * RS_TAPS_THREADS + threadIdx.x);
    if (e >= up * T) return;
    const int p = e / T, k = e - p * T;
    const long long num = (long long)(half - k) * up + p;       // tau = num / up, |tau| <= half iff |num| <= half up
    double h = 0.0;
    if (num <= (long long)half * up && -num <= (long long)half * up) {
        const double tau = (double)num / (double)up;
        const double xs = c * tau, pix = M_PI * xs;
        const double s = xs == 0.0 ? 1.0 : sin(pix) / pix;
        const double r = tau / (double)half;
        const double w = rs_i0(beta * sqrt(fmax(0.0, 1.0 - r * r)));
        h = c * s * w / rs_i0(beta);
    }
    taps[e] = (float)h;
}

// sum_{k = k_lo .. k_hi - 1} tp[k] xp[k] in fp64, ascending k
__device__ __forceinline__ double rs_dot(const float *__restrict__ tp, const float *__restrict__ xr, long long x0, int k_lo, int k_hi)
{
    double acc = 0.0;
#pragma unroll 4
    for (int k = k_lo; k < k_hi; ++k) acc = fma((double)tp[k], (double)xr[x0 + k], acc);
    return acc;
}

template <bool LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_rows_kernel(const float *__restrict__ x, long long x_stride, long long b0,
                                                                   long long n_in, int up, int down, int half,
                                                                   const float *__restrict__ taps, float *__restrict__ y,
                                                                   long long y_stride, long long n_out)
{
    extern __shared__ float rs_tab[];
    const int tid = (int)threadIdx.x;
    const int T = 2 * half + 1;
    if (LDS) {                                                  // the table, from any 4-byte boundary
        const int nt = up * T;
        const RowsSpan s = rows_span(taps, nt);
        if (tid < s.head) rs_tab[tid] = taps[tid];
        const float4 *v = (const float4 *)(taps + s.head);
        for (int i = tid; i < s.nvec; i += RS_THREADS) {
            const float4 q = v[i];
            float *d = rs_tab + s.head + 4 * i;
            d[0] = q.x;
            d[1] = q.y;
            d[2] = q.z;
            d[3] = q.w;
        }
        if (tid < s.tail) rs_tab[s.head + 4 * s.nvec + tid] = taps[s.head + 4 * s.nvec + tid];
        __syncthreads();
    }
    const size_t b = (size_t)b0 + blockIdx.y;
    const float *xr = x + b * (size_t)x_stride;
    float *yr = y + b * (size_t)y_stride;
    const long long m0 = (long long)blockIdx.x * MX_RESAMPLE_OUT_TILE + tid;
    for (int j = 0; j < RS_PER_THREAD; ++j) {
        const long long m = m0 + (long long)j * RS_THREADS;
        if (m >= n_out) break;
        const long long md = m * down, i0 = md / up;            // i0 <= n_in - 1 since (n_out - 1) down < n_in up
        const int p = (int)(md - i0 * up);
        const long long lo = (long long)half - i0, hi = n_in + half - i0;
        const int k_lo = lo > 0 ? (int)lo : 0, k_hi = hi < T ? (int)hi : T;
        double acc;
        if (LDS)
            acc = rs_dot(rs_tab + p * T, xr, i0 - half, k_lo, k_hi);
        else
            acc = rs_dot(taps + (size_t)p * T, xr, i0 - half, k_lo, k_hi);
        yr[m] = (float)acc;
    }
}

// C ABI (resample_abi.h) -----------------------------------------------------------------------
static int64_t rs_gcd(int64_t a, int64_t b)
{
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

static inline double rs_cutoff(int64_t up, int64_t down, double rolloff)
{
    return rolloff * (up < down ? (double)up / (double)down : 1.0);
}

static inline bool rs_filter_ok(double rolloff, double beta)
{
    return rolloff > 0.0 && rolloff <= 1.0 && beta >= 0.0;
}

// the limits on (up, down, T) that the plan, the table and the conversion share
static int rs_table_limits(int64_t up, int64_t down, int64_t T)
{
    if (up > MX_RESAMPLE_MAX_FACTOR || down > MX_RESAMPLE_MAX_FACTOR || T > MX_RESAMPLE_MAX_TAPS || up * T > MX_RESAMPLE_MAX_TABLE)
        return MX_ERR_UNSUPPORTED;
    return MX_OK;
}

// n_out and the number of tiles of rows of n_in samples; up, down <= MX_RESAMPLE_MAX_FACTOR
static int rs_out_length(int64_t n_in, int64_t up, int64_t down, int64_t &n_out, int64_t &tiles)
{
    if (n_in >= (MX_RESAMPLE_MAX_SPAN + up - 1) / up) return MX_ERR_UNSUPPORTED;      // n_in up >= 2^62
    n_out = (n_in * up + down - 1) / down;
    tiles = (n_out + MX_RESAMPLE_OUT_TILE - 1) / MX_RESAMPLE_OUT_TILE;
    return tiles > 2147483647LL ? MX_ERR_UNSUPPORTED : MX_OK;
}

static inline int rs_route(int64_t table_floats)
{
    return 4 * table_floats <= MX_RESAMPLE_LDS_TABLE_BYTES ? MX_RESAMPLE_ROUTE_LDS : MX_RESAMPLE_ROUTE_L2;
}

MX_EXPORT int mx_resample_plan(int64_t sr_in, int64_t sr_out, int32_t zeros, double rolloff, double beta, int64_t n_in, int32_t *up,
                               int32_t *down, int32_t *half, int64_t *n_out, int64_t *table_floats, int32_t *route)
{
    if (!up || !down || !half || !n_out || !table_floats || !route) return MX_ERR_ARG;
    if (sr_in < 1 || sr_out < 1 || zeros < 1 || !rs_filter_ok(rolloff, beta) || n_in < 1) return MX_ERR_ARG;
    if (beta > MX_RESAMPLE_MAX_BETA) return MX_ERR_UNSUPPORTED;
    const int64_t g = rs_gcd(sr_in, sr_out), u = sr_out / g, d = sr_in / g;
    if (u > MX_RESAMPLE_MAX_FACTOR || d > MX_RESAMPLE_MAX_FACTOR) return MX_ERR_UNSUPPORTED;
    const double hf = ceil((double)zeros / rs_cutoff(u, d, rolloff));
    if (!(hf <= (double)MX_RESAMPLE_MAX_TAPS)) return MX_ERR_UNSUPPORTED;
    const int64_t h = (int64_t)hf, T = 2 * h + 1;
    int rc = rs_table_limits(u, d, T);
    if (rc != MX_OK) return rc;
    int64_t no, tiles;
    rc = rs_out_length(n_in, u, d, no, tiles);
    if (rc != MX_OK) return rc;
    *up = (int32_t)u;
    *down = (int32_t)d;
    *half = (int32_t)h;
    *n_out = no;
    *table_floats = u * T;
    *route = rs_route(u * T);
    return MX_OK;
}

MX_EXPORT int mx_resample_taps(int32_t up, int32_t down, int32_t half, double rolloff, double beta, float *taps, void *stream)
{
    if (!taps || up < 1 || down < 1 || half < 1 || rs_gcd(up, down) != 1 || !rs_filter_ok(rolloff, beta)) return MX_ERR_ARG;
    if (beta > MX_RESAMPLE_MAX_BETA) return MX_ERR_UNSUPPORTED;
    const int64_t T = 2 * (int64_t)half + 1;
    const int rc = rs_table_limits(up, down, T);
    if (rc != MX_OK) return rc;
    const unsigned blocks = (unsigned)((up * T + RS_TAPS_THREADS - 1) / RS_TAPS_THREADS);
    hipLaunchKernelGGL(resample_taps_kernel, dim3(blocks), dim3(RS_TAPS_THREADS), 0, (hipStream_t)stream, (int)up, (int)half,
                       rs_cutoff(up, down, rolloff), beta, taps);
    return mx_launch_status();
}

MX_EXPORT int mx_resample_rows(const float *x, int64_t x_stride, int64_t B, int64_t n_in, int32_t up, int32_t down, int32_t half,
                               const float *taps, float *y, int64_t y_stride, int64_t n_out, void *stream)
{
    static MxLdsLatch latch;
    if (!taps || rows_check(x, x_stride, B, n_in) != MX_OK || rows_check(y, y_stride, B, n_out) != MX_OK) return MX_ERR_ARG;
    if (up < 1 || down < 1 || half < 1 || rs_gcd(up, down) != 1) return MX_ERR_ARG;
    const int64_t T = 2 * (int64_t)half + 1;
    int rc = rs_table_limits(up, down, T);
    if (rc != MX_OK) return rc;
    int64_t no, tiles;
    rc = rs_out_length(n_in, up, down, no, tiles);
    if (rc != MX_OK) return rc;
    if (n_out != no) return MX_ERR_ARG;
    const RowsRange out = rows_range(y, y_stride, B, n_out);
    const RowsRange in[2] = {rows_range(x, x_stride, B, n_in), rows_flat(taps, up * T, 4)};
    if (rows_any_overlap(&out, 1, in, 2)) return MX_ERR_ARG;
    const bool lds = rs_route(up * T) == MX_RESAMPLE_ROUTE_LDS;
    const size_t lds_bytes = lds ? (size_t)(4 * up * T) : 0;
    if (lds) {
        rc = mx_set_dyn_lds(latch, (const void *)resample_rows_kernel<true>, MX_RESAMPLE_LDS_TABLE_BYTES);
        if (rc != MX_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int64_t b0 = 0; b0 < B; b0 += RS_MAX_ROWS) {
        const unsigned rows = (unsigned)(B - b0 < RS_MAX_ROWS ? B - b0 : RS_MAX_ROWS);
        const dim3 grid((unsigned)tiles, rows);
        if (lds)
            hipLaunchKernelGGL(resample_rows_kernel<true>, grid, dim3(RS_THREADS), lds_bytes, st, x, (long long)x_stride,
                               (long long)b0, (long long)n_in, (int)up, (int)down, (int)half, taps, y, (long long)y_stride,
                               (long long)n_out);
        else
            hipLaunchKernelGGL(resample_rows_kernel<false>, grid, dim3(RS_THREADS), 0, st, x, (long long)x_stride, (long long)b0,
                               (long long)n_in, (int)up, (int)down, (int)half, taps, y, (long long)y_stride, (long long)n_out);
    }
    return mx_launch_status();
}
