// fir_match.hip -- K21: one short least-squares FIR per clip that carries a rendered wet (y_hat = x) onto a recorded one (y),
// forward and backward -- no counterpart in the reference (include/modex_hip.h, K21, has the definition).
//
//     R[d] = sum_n x[n] x[n + d],  b[j] = sum_n x[n + c - j] y[n],  E = sum_n y[n]^2;   A = toeplitz(R) + (eps + ridge R[0]) I
//     h = A^-1 b (fp64 Cholesky), rounded once;   z[n] = sum_k h[k] x[n + c - k]
//     gh[k] = sum_n dz[n] x[n + c - k],  u = A^-1 gh,  s = the 2K - 1 lags of h (x) u + u (x) h (+ 2 ridge <u, h> at lag 0)
//     dy_hat[i] = sum_k h[k] dz[i + k - c] + sum_k u[k] y[i + k - c] - sum_d s[d] x[i + d]
//
// The grid conventions of gain_match.hip: grid (chunk, row), 256 threads, a workgroup owns FM_CHUNK = 2048 samples of one row;
// rows a row stride apart are read in place wherever they start; no atomics.  Every array is staged once per workgroup in
// LDS with its halo of up to K - 1 samples a side, by dword loads behind an index test: what lies outside [0, N) of the
// row reads as 0 and is never loaded.
//
// fm_partials_kernel<FWD>   a LAG PER LANE (pair_align.hip is the precedent): the 2K outputs R[0..K), b[0..K) (backward: the K
//     of gh) sit on P = the next power of two lanes; a wave holds 64 / P such groups and the 4 * 64 / P groups of the
//     workgroup take the chunk's samples round robin.  Per product two ds_read_b32 (x[n] or y[n]: one address per group,
//     a broadcast; x[n + lag]: consecutive lanes, consecutive banks), two conversions and one fp64 fma -- the product of two
//     converted fp32 values is exact.  Fixed order: a lane over its samples, the groups of a wave by butterfly, the four
//     waves 0 + 1 + 2 + 3 through LDS.  E as in gain_match.hip.
// fm_solve_kernel           one wave per row.  Lanes m and m + 64 add the chunks' partials in the order 0, 1, 2, ..; lane i
//     owns row i of A in LDS (pitch 33 doubles): right-looking Cholesky, the two triangular solves with the right-hand side
//     one element a lane, exchanged by __shfl.  The guards are wave-uniform.
// fm_bwd_solve_kernel       the same reduction of gh, A built and factored again from the forward's R (K^3 / 6 flops: not
//     worth a (B, K, K) buffer), u by the same two solves, s by one lag per lane.
// fm_apply_kernel, fm_bwd_apply_kernel   thread t forms samples t, t + 256, .. of the chunk in fp64 from LDS (consecutive
//     lanes, consecutive banks), rounds once into an LDS row of results, and the workgroup stores that row as a scalar head up
//     to the first 16-byte boundary of the output, float4s, and a scalar tail (rows_span's rule). Coefficients are read from
//     LDS at one address a wave (a broadcast); one that is exactly 0 is skipped, so the identity filter copies.
#include "rows_common.h"

#define FM_THREADS 256
#define FM_CHUNK MX_FIR_CHUNK
#define FM_MAXK MX_FIR_MAX_TAPS
#define FM_MAX_N (1ll << 24)
#define FM_MAX_B 65535
#define FM_HALO (FM_MAXK - 1)
#define FM_PITCH (FM_MAXK + 1)

static_assert(FM_CHUNK % 4 == 0 && FM_CHUNK % FM_THREADS == 0, "every chunk of a row shares the row's head");
static_assert(2 * FM_MAXK <= MX_WAVE, "R and b of one row fit the lanes of a wave");

// row[gi] for gi in [0, N), else 0 -- never a load outside the row
__device__ __forceinline__ float fm_at(const float *__restrict__ row, int gi, int N)
{
    return (gi >= 0 && gi < N) ? row[gi] : 0.0f;
}

// dst[i] = row[g0 + i], i in [0, count), by the whole workgroup
__device__ __forceinline__ void fm_stage(float *dst, const float *__restrict__ row, int g0, int count, int N)
{
    for (int i = (int)threadIdx.x; i < count; i += FM_THREADS) dst[i] = fm_at(row, g0 + i, N);
}

// FWD: partials[b, chunk, 0 : 2K + 1] = R, b, E of the chunk with q = y;  !FWD: partials[b, chunk, 0 : K] = gh with q = dz
template <bool FWD>
__global__ __launch_bounds__(FM_THREADS) void fm_partials_kernel(
    const float *__restrict__ x, long long x_stride, const float *__restrict__ q, long long q_stride, int N, int K, int c,
    double *__restrict__ partials)
{
    // sm[0 : len + 2 (K - 1)] = x[n0 - (K - 1) ..], sm[FM_XS : FM_XS + len] = q[n0 ..]
    constexpr int FM_XS = FM_CHUNK + 2 * FM_HALO;
    __shared__ float sm[FM_XS + FM_CHUNK];
    __shared__ double part[4][MX_WAVE];
    __shared__ double red[4];
    const int tid = (int)threadIdx.x, lane = tid & (MX_WAVE - 1), wave = tid / MX_WAVE;
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * FM_CHUNK;
    const int len = min(FM_CHUNK, N - n0);                          // >= 1: the grid has ceil(N / FM_CHUNK) chunks
    fm_stage(sm, x + b * (size_t)x_stride, n0 - (K - 1), len + 2 * (K - 1), N);
    fm_stage(sm + FM_XS, q + b * (size_t)q_stride, n0, len, N);
    __syncthreads();
    const int nout = FWD ? 2 * K : K;
    int P = 1;
    while (P < nout) P <<= 1;                                       // <= 64
    const int m = lane & (P - 1), groups = MX_WAVE / P, first = wave * groups + lane / P, step = 4 * groups;
    // output m multiplies sm[ia + n] by sm[ib + n] over the chunk's samples n
    int ia, ib;
    if (FWD && m < K) {                                             // R[m] = sum x[n] x[n + m]
        ia = K - 1;
        ib = K - 1 + m;
    } else {                                                        // b[j] or gh[j] = sum q[n] x[n + c - j]
        const int j = FWD ? m - K : m;
        ia = FM_XS;
        ib = K - 1 + c - j;
    }
    double acc = 0.0;
    if (m < nout)
        for (int n = first; n < len; n += step) acc = fma((double)sm[ia + n], (double)sm[ib + n], acc);
    for (int o = P; o < MX_WAVE; o <<= 1) acc += __shfl_xor(acc, o, MX_WAVE);
    part[wave][lane] = acc;
    double e = 0.0;
    if (FWD) {
        for (int n = tid; n < len; n += FM_THREADS) {
            const double v = (double)sm[FM_XS + n];
            e = fma(v, v, e);
        }
        e = block256_sum_f64(e, red);                               // its barriers publish part[][] too
    } else {
        __syncthreads();
    }
    double *o = partials + (b * gridDim.x + blockIdx.x) * (size_t)(FWD ? 2 * K + 1 : K);
    if (tid < nout) o[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    if (FWD && tid == 0) o[2 * K] = e;
}

// A = toeplitz(R) + lambda I into As (lane i writes row i), then its Cholesky factor in place (lower triangle, L[j][j] on
// the diagonal).  One wave; returns false, on every lane, at the first pivot that is not positive or not finite.
__device__ __forceinline__ bool fm_factor(double (*As)[FM_PITCH], const double *R, int K, double lambda, int lane)
{
    if (lane < K)
        for (int j = 0; j < K; ++j) As[lane][j] = R[abs(lane - j)] + (lane == j ? lambda : 0.0);
    __syncthreads();
    for (int j = 0; j < K; ++j) {
        const double d = As[j][j];
        if (!(d > 0.0) || !(d < INFINITY)) return false;            // the same d on every lane
        const double r = sqrt(d);
        __syncthreads();                                            // everyone has read the pivot
        if (lane == j) As[j][j] = r;
        if (lane > j && lane < K) As[lane][j] = As[lane][j] / r;
        __syncthreads();
        if (lane > j && lane < K) {
            const double l = As[lane][j];
            for (int k = j + 1; k <= lane; ++k) As[lane][k] = fma(-l, As[k][j], As[lane][k]);
        }
        __syncthreads();
    }
    return true;
}

// A v = rhs for the factored A: lane i holds rhs[i] and returns v[i] (lanes >= K: 0)
__device__ __forceinline__ double fm_solve(double (*As)[FM_PITCH], int K, int lane, double v)
{
    for (int j = 0; j < K; ++j) {                                   // L w = rhs
        const double w = __shfl(v, j, MX_WAVE) / As[j][j];
        if (lane == j) v = w;
        if (lane > j && lane < K) v = fma(-As[lane][j], w, v);
    }
    for (int j = K - 1; j >= 0; --j) {                              // L^T v = w
        const double w = __shfl(v, j, MX_WAVE) / As[j][j];
        if (lane == j) v = w;
        if (lane < j) v = fma(-As[j][lane], w, v);
    }
    return lane < K ? v : 0.0;
}

__global__ __launch_bounds__(MX_WAVE) void fm_solve_kernel(
    const double *__restrict__ partials, int n_chunks, int K, int c, double ridge, double eps, double max_gain,
    float *__restrict__ taps, double *__restrict__ sums, int *__restrict__ flags)
{
    __shared__ double As[FM_MAXK][FM_PITCH];
    __shared__ double tot[2 * FM_MAXK + 1];
    const int lane = (int)threadIdx.x, W = 2 * K + 1;
    const size_t b = blockIdx.x;
    const double *pr = partials + b * (size_t)n_chunks * W;
    for (int m = lane; m < W; m += MX_WAVE) {
        double a = 0.0;
        for (int k = 0; k < n_chunks; ++k) a += pr[(size_t)k * W + m];
        tot[m] = a;
        sums[b * W + m] = a;
    }
    __syncthreads();
    int flag = 0;
    double h = 0.0;
    if (!fm_factor(As, tot, K, eps + ridge * tot[0], lane)) {
        flag = 1;
    } else {
        h = fm_solve(As, K, lane, lane < K ? tot[K + lane] : 0.0);
        if (!(wave_sum_f64(fabs(h)) <= max_gain)) flag = 2;
    }
    if (flag) h = lane == c ? 1.0 : 0.0;
    if (lane < K) taps[b * K + lane] = (float)h;
    if (lane == 0) flags[b] = flag;
}

__global__ __launch_bounds__(MX_WAVE) void fm_bwd_solve_kernel(
    const double *__restrict__ partials, const double *__restrict__ sums, const float *__restrict__ taps,
    const int *__restrict__ flags, int n_chunks, int K, double ridge, double eps, double *__restrict__ u,
    double *__restrict__ s)
{
    __shared__ double As[FM_MAXK][FM_PITCH];
    __shared__ double R[FM_MAXK], hs[FM_MAXK], us[FM_MAXK];
    const int lane = (int)threadIdx.x;
    const size_t b = blockIdx.x;
    double g = 0.0;
    if (lane < K) {
        const double *pr = partials + b * (size_t)n_chunks * K;
        for (int k = 0; k < n_chunks; ++k) g += pr[(size_t)k * K + lane];
        R[lane] = sums[b * (2 * K + 1) + lane];
        hs[lane] = (double)taps[b * K + lane];
    }
    __syncthreads();
    double v = 0.0;
    if (flags[b] == 0 && fm_factor(As, R, K, eps + ridge * R[0], lane)) v = fm_solve(As, K, lane, g);
    if (lane < K) {
        us[lane] = v;
        u[b * K + lane] = v;
    }
    __syncthreads();
    if (lane < 2 * K - 1) {
        const int d = abs(lane - (K - 1));
        double acc = 0.0, dot = 0.0;
        for (int j = 0; j + d < K; ++j) acc = fma(hs[j + d], us[j], fma(us[j + d], hs[j], acc));
        if (d == 0) {
            for (int j = 0; j < K; ++j) dot = fma(us[j], hs[j], dot);
            acc = fma(2.0 * ridge, dot, acc);
        }
        s[b * (2 * K - 1) + lane] = acc;
    }
}

// o[0 : len] = res[0 : len] (LDS, 16-byte aligned): scalar head, float4s, scalar tail
__device__ __forceinline__ void fm_store(float *o, const float *res, int len)
{
    const int tid = (int)threadIdx.x;
    const RowsSpan sp = rows_span(o, len);
    if (tid < sp.head) o[tid] = res[tid];
    float4 *ov = reinterpret_cast<float4 *>(o + sp.head);
    for (int i = tid; i < sp.nvec; i += FM_THREADS) {
        const float *r = res + sp.head + 4 * i;
        ov[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
    if (tid < sp.tail) {
        const int i = sp.head + 4 * sp.nvec + tid;
        o[i] = res[i];
    }
}

// acc += sum_k coef[k] v[k * dir], k = 0 .. n - 1, zero coefficients skipped (coef: one LDS address a wave)
__device__ __forceinline__ double fm_dot(const double *coef, int n, const float *v, int dir, double acc)
{
    for (int k = 0; k < n; ++k) {
        const double h = coef[k];
        if (h != 0.0) acc = fma(h, (double)v[k * dir], acc);
    }
    return acc;
}

__global__ __launch_bounds__(FM_THREADS) void fm_apply_kernel(
    const float *__restrict__ x, long long x_stride, const float *__restrict__ taps, int N, int K, int c,
    float *__restrict__ z, long long z_stride)
{
    __shared__ float xs[FM_CHUNK + FM_HALO];                        // xs[i] = x[n0 + c - (K - 1) + i]
    __shared__ __attribute__((aligned(16))) float res[FM_CHUNK];
    __shared__ double hs[FM_MAXK];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * FM_CHUNK;
    const int len = min(FM_CHUNK, N - n0);
    fm_stage(xs, x + b * (size_t)x_stride, n0 + c - (K - 1), len + K - 1, N);
    if (tid < K) hs[tid] = (double)taps[b * K + tid];
    __syncthreads();
    // z[n0 + m] = sum_k h[k] xs[m + (K - 1) - k]
    for (int m = tid; m < len; m += FM_THREADS) res[m] = (float)fm_dot(hs, K, xs + m + K - 1, -1, 0.0);
    __syncthreads();
    fm_store(z + b * (size_t)z_stride + n0, res, len);
}

__global__ __launch_bounds__(FM_THREADS) void fm_bwd_apply_kernel(
    const float *__restrict__ dz, long long dz_stride, const float *__restrict__ y, long long y_stride,
    const float *__restrict__ x, long long x_stride, const float *__restrict__ taps, const double *__restrict__ u,
    const double *__restrict__ s, int N, int K, int c, float *__restrict__ dy_hat, long long dy_hat_stride)
{
    __shared__ float ds[FM_CHUNK + FM_HALO], ys[FM_CHUNK + FM_HALO];    // [i] = dz, y[n0 - c + i]
    __shared__ float xs[FM_CHUNK + 2 * FM_HALO];                        // [i] = x[n0 - (K - 1) + i]
    __shared__ __attribute__((aligned(16))) float res[FM_CHUNK];
    __shared__ double hs[FM_MAXK], us[FM_MAXK], ss[2 * FM_MAXK - 1];
    const int tid = (int)threadIdx.x;
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * FM_CHUNK;
    const int len = min(FM_CHUNK, N - n0);
    fm_stage(ds, dz + b * (size_t)dz_stride, n0 - c, len + K - 1, N);
    fm_stage(ys, y + b * (size_t)y_stride, n0 - c, len + K - 1, N);
    fm_stage(xs, x + b * (size_t)x_stride, n0 - (K - 1), len + 2 * (K - 1), N);
    if (tid < K) {
        hs[tid] = (double)taps[b * K + tid];
        us[tid] = u[b * K + tid];
    }
    if (tid < 2 * K - 1) ss[tid] = -s[b * (2 * K - 1) + tid];       // subtracted: the sign is exact
    __syncthreads();
    for (int m = tid; m < len; m += FM_THREADS) {
        double acc = fm_dot(hs, K, ds + m, 1, 0.0);                 // sum_k h[k] dz[i + k - c]
        acc = fm_dot(us, K, ys + m, 1, acc);                        // sum_k u[k] y[i + k - c]
        acc = fm_dot(ss, 2 * K - 1, xs + m, 1, acc);                // - sum_d s[d] x[i + d], d = -(K - 1) ..
        res[m] = (float)acc;
    }
    __syncthreads();
    fm_store(dy_hat + b * (size_t)dy_hat_stride + n0, res, len);
}

// C ABI ---------------------------------------------------------------------------------------
// K, then the centre, then the sizes
static int fm_check_dims(int64_t B, int64_t N, int64_t K, int64_t centre, bool has_centre)
{
    if (K < 1 || K > FM_MAXK) return MX_ERR_UNSUPPORTED;
    if (has_centre && (centre < 0 || centre >= K)) return MX_ERR_ARG;
    return (N > FM_MAX_N || B > FM_MAX_B) ? MX_ERR_UNSUPPORTED : MX_OK;
}

static bool fm_bad_ridge_eps(double ridge, double eps)
{
    return !(ridge >= 0.0) || !(ridge < 1e300) || !(eps > 0.0) || !(eps < 1e300);
}

static int64_t fm_chunks(int64_t N)
{
    return (N + FM_CHUNK - 1) / FM_CHUNK;
}

static dim3 fm_grid(int64_t B, int64_t N)
{
    return dim3((unsigned)fm_chunks(N), (unsigned)B);
}

MX_EXPORT int mx_fir_match_partials(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                                    int64_t N, int64_t K, int64_t centre, double *partials, void *stream)
{
    if (!partials || rows_check(y_hat, y_hat_stride, B, N) || rows_check(y, y_stride, B, N)) return MX_ERR_ARG;
    if (const int rc = fm_check_dims(B, N, K, centre, true)) return rc;
    const RowsRange out[1] = {rows_flat(partials, B * fm_chunks(N) * (2 * K + 1), 8)};
    const RowsRange in[2] = {rows_range(y_hat, y_hat_stride, B, N), rows_range(y, y_stride, B, N)};
    if (rows_any_overlap(out, 1, in, 2)) return MX_ERR_ARG;
    hipLaunchKernelGGL(fm_partials_kernel<true>, fm_grid(B, N), dim3(FM_THREADS), 0, (hipStream_t)stream, y_hat,
                       (long long)y_hat_stride, y, (long long)y_stride, (int)N, (int)K, (int)centre, partials);
    return mx_launch_status();
}

MX_EXPORT int mx_fir_match_solve(const double *partials, int64_t B, int64_t n_chunks, int64_t K, int64_t centre, double ridge,
                                 double eps, double max_gain, float *taps, double *sums, int32_t *flags, void *stream)
{
    if (!partials || !taps || !sums || !flags || B < 1 || n_chunks < 1) return MX_ERR_ARG;
    if (const int rc = fm_check_dims(B, n_chunks, K, centre, true)) return rc;
    if (n_chunks > fm_chunks(FM_MAX_N)) return MX_ERR_UNSUPPORTED;
    if (fm_bad_ridge_eps(ridge, eps) || !(max_gain >= 1.0) || !(max_gain < 1e300)) return MX_ERR_ARG;
    const RowsRange out[3] = {rows_flat(taps, B * K, 4), rows_flat(sums, B * (2 * K + 1), 8), rows_flat(flags, B, 4)};
    const RowsRange in[1] = {rows_flat(partials, B * n_chunks * (2 * K + 1), 8)};
    if (rows_any_overlap(out, 3, in, 1)) return MX_ERR_ARG;
    hipLaunchKernelGGL(fm_solve_kernel, dim3((unsigned)B), dim3(MX_WAVE), 0, (hipStream_t)stream, partials, (int)n_chunks,
                       (int)K, (int)centre, ridge, eps, max_gain, taps, sums, (int *)flags);
    return mx_launch_status();
}

MX_EXPORT int mx_fir_match_apply(const float *x, int64_t x_stride, const float *taps, int64_t B, int64_t N, int64_t K,
                                 int64_t centre, float *z, int64_t z_stride, void *stream)
{
    if (!taps || rows_check(x, x_stride, B, N) || rows_check(z, z_stride, B, N)) return MX_ERR_ARG;
    if (const int rc = fm_check_dims(B, N, K, centre, true)) return rc;
    const RowsRange out[1] = {rows_range(z, z_stride, B, N)};
    const RowsRange in[2] = {rows_range(x, x_stride, B, N), rows_flat(taps, B * K, 4)};
    if (rows_any_overlap(out, 1, in, 2)) return MX_ERR_ARG;
    hipLaunchKernelGGL(fm_apply_kernel, fm_grid(B, N), dim3(FM_THREADS), 0, (hipStream_t)stream, x, (long long)x_stride, taps,
                       (int)N, (int)K, (int)centre, z, (long long)z_stride);
    return mx_launch_status();
}

MX_EXPORT int mx_fir_match_bwd_partials(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride,
                                        int64_t B, int64_t N, int64_t K, int64_t centre, double *partials, void *stream)
{
    if (!partials || rows_check(dz, dz_stride, B, N) || rows_check(y_hat, y_hat_stride, B, N)) return MX_ERR_ARG;
    if (const int rc = fm_check_dims(B, N, K, centre, true)) return rc;
    const RowsRange out[1] = {rows_flat(partials, B * fm_chunks(N) * K, 8)};
    const RowsRange in[2] = {rows_range(dz, dz_stride, B, N), rows_range(y_hat, y_hat_stride, B, N)};
    if (rows_any_overlap(out, 1, in, 2)) return MX_ERR_ARG;
    hipLaunchKernelGGL(fm_partials_kernel<false>, fm_grid(B, N), dim3(FM_THREADS), 0, (hipStream_t)stream, y_hat,
                       (long long)y_hat_stride, dz, (long long)dz_stride, (int)N, (int)K, (int)centre, partials);
    return mx_launch_status();
}

MX_EXPORT int mx_fir_match_bwd_solve(const double *partials, const double *sums, const float *taps, const int32_t *flags,
                                     int64_t B, int64_t n_chunks, int64_t K, double ridge, double eps, double *u, double *s,
                                     void *stream)
{
    if (!partials || !sums || !taps || !flags || !u || !s || B < 1 || n_chunks < 1) return MX_ERR_ARG;
    if (const int rc = fm_check_dims(B, n_chunks, K, 0, false)) return rc;
    if (n_chunks > fm_chunks(FM_MAX_N)) return MX_ERR_UNSUPPORTED;
    if (fm_bad_ridge_eps(ridge, eps)) return MX_ERR_ARG;
    const RowsRange out[2] = {rows_flat(u, B * K, 8), rows_flat(s, B * (2 * K - 1), 8)};
    const RowsRange in[4] = {rows_flat(partials, B * n_chunks * K, 8), rows_flat(sums, B * (2 * K + 1), 8),
                             rows_flat(taps, B * K, 4), rows_flat(flags, B, 4)};
    if (rows_any_overlap(out, 2, in, 4)) return MX_ERR_ARG;
    hipLaunchKernelGGL(fm_bwd_solve_kernel, dim3((unsigned)B), dim3(MX_WAVE), 0, (hipStream_t)stream, partials, sums, taps,
                       (const int *)flags, (int)n_chunks, (int)K, ridge, eps, u, s);
    return mx_launch_status();
}

MX_EXPORT int mx_fir_match_bwd_apply(const float *dz, int64_t dz_stride, const float *y, int64_t y_stride, const float *y_hat,
                                     int64_t y_hat_stride, const float *taps, const double *u, const double *s, int64_t B,
                                     int64_t N, int64_t K, int64_t centre, float *dy_hat, int64_t dy_hat_stride, void *stream)
{
    if (!taps || !u || !s || rows_check(dz, dz_stride, B, N) || rows_check(y, y_stride, B, N)
        || rows_check(y_hat, y_hat_stride, B, N) || rows_check(dy_hat, dy_hat_stride, B, N))
        return MX_ERR_ARG;
    if (const int rc = fm_check_dims(B, N, K, centre, true)) return rc;
    const RowsRange out[1] = {rows_range(dy_hat, dy_hat_stride, B, N)};
    const RowsRange in[6] = {rows_range(dz, dz_stride, B, N), rows_range(y, y_stride, B, N),
                             rows_range(y_hat, y_hat_stride, B, N), rows_flat(taps, B * K, 4), rows_flat(u, B * K, 8),
                             rows_flat(s, B * (2 * K - 1), 8)};
    if (rows_any_overlap(out, 1, in, 6)) return MX_ERR_ARG;
    hipLaunchKernelGGL(fm_bwd_apply_kernel, fm_grid(B, N), dim3(FM_THREADS), 0, (hipStream_t)stream, dz, (long long)dz_stride,
                       y, (long long)y_stride, y_hat, (long long)y_hat_stride, taps, u, s, (int)N, (int)K, (int)centre, dy_hat,
                       (long long)dy_hat_stride);
    return mx_launch_status();
}
