// shaper_match.hip -- K27: one memoryless polynomial curve per clip that carries a rendered wet (y_hat) onto a recorded one
// (y) that went through a saturating stage, forward and backward -- no counterpart in the reference (shaper_match_abi.h has
// the definition and the layout of the sums).
//
// The elementwise kernels: grid (chunk, row), 256 threads, a workgroup owns SH_CHUNK = 2048 samples of one row, walked as in
// gain_match.hip: a scalar head up to the first 16-byte boundary of the LEADING array (the one that is stored where there is
// one, else the first one read), aligned float4s of it, a scalar tail; the other arrays of the same elements through a
// 4-byte-aligned vector type.  They are templates on (order, even), so the powers of t and the sums they feed stay in
// registers: a lane forms t = x / r and t^2, t^3, .. by repeated multiplication and adds only what the order needs.
//
// shaper_s2_kernel            the chunk's sum of x^2 (exact products, fp64) -> slot 0 of the chunk.
// shaper_moments_kernel       every wave re-reduces the row's S2 from slot 0 of all chunks (sh_wave_chunks: the function the
//                             solve uses, so both hold the same r), then the chunk's moments, cross sums and E -> the other slots.
// shaper_solve_kernel         one wave a row: the sums from the chunks, r, and on lane 0 the K x K Cholesky in LDS, the guards.
// shaper_apply_kernel         z = fl32(r C(t)) by Horner; a flagged row is copied.
// shaper_bwd_partials_kernel  the chunk's g_k = sum dz t^(p_k).
// shaper_bwd_solve_kernel     one wave a row: g, A from the forward's sums, u = A^-1 g.
// shaper_bwd_apply_kernel     dy_hat per element from the powers t^0 .. t^(2 p_K - 1); a thread reads dz[i] before it writes
//                             dy_hat[i] and nobody else touches i, so dy_hat may be dz.
// Bound by HBM or launch latency: forward 3 reads + (1 read, 1 write) of B N floats, backward 2 + (3, 1); a few tens of fp64
// operations a sample (two of them divisions).
#include "rows_common.h"
#include "shaper_match_abi.h"

#define SH_THREADS 256
#define SH_CHUNK MX_SHAPER_CHUNK
#define SH_MAXK MX_SHAPER_MAX_ORDER
#define SH_MAX_SUMS (1 + (2 * SH_MAXK - 1) + SH_MAXK + 1)

static_assert(SH_CHUNK % 4 == 0, "every chunk of a row shares the row's head");

// (order, even) -> the powers and the layout of the sums.  Without `even` P is odd (the host rounds an even order down).
template <int P, bool EVEN> struct ShCfg {
    static constexpr int K = EVEN ? P : (P + 1) / 2;                // coefficients
    static constexpr int NM = EVEN ? 2 * P - 1 : P;                 // moments: m = 2 .. 2 P, without `even` the even m only
    static constexpr int NS = 1 + NM + K + 1;                       // S2, moments, b, E
    __host__ __device__ static constexpr int power(int k) { return EVEN ? k + 1 : 2 * k + 1; }
    __host__ __device__ static constexpr bool is_power(int q) { return q >= 1 && q <= P && (EVEN || (q & 1)); }
    __host__ __device__ static constexpr int k_of(int q) { return EVEN ? q - 1 : (q - 1) / 2; }
    __host__ __device__ static constexpr bool is_moment(int q) { return q >= 2 && q <= 2 * P && (EVEN || !(q & 1)); }
    __host__ __device__ static constexpr int m_of(int q) { return EVEN ? q - 2 : (q - 2) / 2; }
};

// the same three numbers at run time (the solves, the host)
struct ShShape { int K, NM, NS, P; bool even; };
__host__ __device__ static inline ShShape sh_shape(int order, int even)
{
    ShShape s;
    s.even = even != 0;
    s.P = s.even ? order : (order & 1 ? order : order - 1);
    s.K = s.even ? s.P : (s.P + 1) / 2;
    s.NM = s.even ? 2 * s.P - 1 : s.P;
    s.NS = 1 + s.NM + s.K + 1;
    return s;
}
__device__ __forceinline__ int sh_power(const ShShape &s, int k) { return s.even ? k + 1 : 2 * k + 1; }
__device__ __forceinline__ int sh_m_of(const ShShape &s, int q) { return s.even ? q - 2 : (q - 2) / 2; }

__device__ __forceinline__ RowsUFloat4 sh_ldu(const float *p) { return *reinterpret_cast<const RowsUFloat4 *>(p); }
__device__ __forceinline__ float4 sh_lda(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// len floats from lead: one(i) for the floats of the head and the tail, four(i) for every aligned group of four at lead + i
template <class One, class Four>
__device__ __forceinline__ void sh_walk(const float *lead, int len, One one, Four four)
{
    const int tid = (int)threadIdx.x;
    const RowsSpan sp = rows_span(lead, len);
    if (tid < sp.head) one(tid);
    for (int i = tid; i < sp.nvec; i += SH_THREADS) four(sp.head + 4 * i);
    if (tid < sp.tail) one(sp.head + 4 * sp.nvec + tid);
}

// n block sums at once; red: 4 n doubles of LDS.  Fixed order: lanes by butterfly, then waves 0 + 1 + 2 + 3.
template <int NV>
__device__ __forceinline__ void sh_block_sums(double (&v)[NV], double *red)
{
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum_f64(v[i]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < NV; ++i) red[4 * i + w] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = ((red[4 * i] + red[4 * i + 1]) + red[4 * i + 2]) + red[4 * i + 3];
}

// one wave: slot s of a row's chunks, lane l taking chunks l, l + 64, .. in ascending order, then the butterfly.  Every
// wave that calls it on the same row holds the same bits.
__device__ __forceinline__ double sh_wave_chunks(const double *pr, int n_chunks, int n_sums, int s)
{
    double acc = 0.0;
    for (int k = (int)(threadIdx.x & 63); k < n_chunks; k += 64) acc += pr[(size_t)k * n_sums + s];
    return wave_sum_f64(acc);
}

// r = fl32(sqrt(S2 / N)); bad: S2 or r not positive or not finite (then r = 1)
__device__ __forceinline__ float sh_scale(double S2, int N, bool &bad)
{
    const float r = (float)sqrt(S2 / (double)N);
    bad = !(S2 > 0.0) || !(S2 < HUGE_VAL) || !(r > 0.0f) || !(r < HUGE_VALF);
    return bad ? 1.0f : r;
}

__global__ __launch_bounds__(SH_THREADS) void shaper_s2_kernel(const float *__restrict__ y_hat, long long y_hat_stride, int N,
                                                               int n_sums, double *__restrict__ partials)
{
    __shared__ double red[4];
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * SH_CHUNK;
    const int len = min(SH_CHUNK, N - n0);                          // >= 1: the grid has ceil(N / SH_CHUNK) chunks
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    double a = 0.0;
    sh_walk(p, len,
            [&](int i) { const double u = (double)p[i]; a = fma(u, u, a); },
            [&](int i) {
                const float4 u = sh_lda(p + i);
                a = fma((double)u.x, (double)u.x, a);
                a = fma((double)u.y, (double)u.y, a);
                a = fma((double)u.z, (double)u.z, a);
                a = fma((double)u.w, (double)u.w, a);
            });
    a = block256_sum_f64(a, red);
    if (threadIdx.x == 0) partials[(b * gridDim.x + blockIdx.x) * (size_t)n_sums] = a;
}

// one sample into the lane's sums: v[0] is unused here (slot 0 is S2), v[1 + m] the moments, then b, then E
template <int P, bool EVEN>
__device__ __forceinline__ void sh_moments_one(float xf, float yf, double r, double (&v)[ShCfg<P, EVEN>::NS])
{
    using C = ShCfg<P, EVEN>;
    const double t = (double)xf / r, yr = (double)yf / r;
    double pw = t;
#pragma unroll
    for (int q = 1; q <= 2 * P; ++q) {
        if (q > 1) pw = pw * t;                                     // t^q
        if (C::is_power(q)) v[1 + C::NM + C::k_of(q)] = fma(pw, yr, v[1 + C::NM + C::k_of(q)]);
        if (C::is_moment(q)) v[1 + C::m_of(q)] += pw;
    }
    v[C::NS - 1] = fma((double)yf, (double)yf, v[C::NS - 1]);
}

template <int P, bool EVEN>
__global__ __launch_bounds__(SH_THREADS) void shaper_moments_kernel(const float *__restrict__ y_hat, long long y_hat_stride,
                                                                    const float *__restrict__ y, long long y_stride, int N,
                                                                    double *partials)
{
    using C = ShCfg<P, EVEN>;
    __shared__ double red[4 * C::NS];
    const size_t b = blockIdx.y;
    const int n_chunks = (int)gridDim.x;
    double *pr = partials + b * (size_t)n_chunks * C::NS;
    bool bad;
    const double r = (double)sh_scale(sh_wave_chunks(pr, n_chunks, C::NS, 0), N, bad);
    const int n0 = (int)blockIdx.x * SH_CHUNK;
    const int len = min(SH_CHUNK, N - n0);
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    const float *q = y + b * (size_t)y_stride + n0;
    double v[C::NS];
#pragma unroll
    for (int i = 0; i < C::NS; ++i) v[i] = 0.0;
    sh_walk(p, len,
            [&](int i) { sh_moments_one<P, EVEN>(p[i], q[i], r, v); },
            [&](int i) {
                const float4 u = sh_lda(p + i);
                const RowsUFloat4 w = sh_ldu(q + i);
                sh_moments_one<P, EVEN>(u.x, w.x, r, v);
                sh_moments_one<P, EVEN>(u.y, w.y, r, v);
                sh_moments_one<P, EVEN>(u.z, w.z, r, v);
                sh_moments_one<P, EVEN>(u.w, w.w, r, v);
            });
    sh_block_sums<C::NS>(v, red);
    if (threadIdx.x == 0) {
        double *o = pr + (size_t)blockIdx.x * C::NS;
#pragma unroll
        for (int i = 1; i < C::NS; ++i) o[i] = v[i];                // slot 0 holds the chunk's S2
    }
}

// lane 0, in LDS: A = the moments with the diagonal times (1 + ridge), its Cholesky factor in place (lower triangle), and
// x = A^-1 rhs in place.  false: a pivot that is not positive or not finite.
__device__ __forceinline__ bool sh_cholesky_solve(const ShShape &s, const double *moments, double ridge, double (*A)[SH_MAXK],
                                                  double *x)
{
    const int K = s.K;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) {
            const double m = moments[sh_m_of(s, sh_power(s, i) + sh_power(s, j))];
            A[i][j] = i == j ? m * (1.0 + ridge) : m;
        }
    for (int j = 0; j < K; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
        if (!(d > 0.0) || !(d < HUGE_VAL)) return false;
        const double l = sqrt(d);
        A[j][j] = l;
        for (int i = j + 1; i < K; ++i) {
            double a = A[i][j];
            for (int k = 0; k < j; ++k) a -= A[i][k] * A[j][k];
            A[i][j] = a / l;
        }
    }
    for (int i = 0; i < K; ++i) {                                   // L w = rhs
        double a = x[i];
        for (int k = 0; k < i; ++k) a -= A[i][k] * x[k];
        x[i] = a / A[i][i];
    }
    for (int i = K - 1; i >= 0; --i) {                              // L^T x = w
        double a = x[i];
        for (int k = i + 1; k < K; ++k) a -= A[k][i] * x[k];
        x[i] = a / A[i][i];
    }
    return true;
}

__global__ __launch_bounds__(64) void shaper_solve_kernel(const double *__restrict__ partials, int N, int n_chunks, int order,
                                                          int even, double ridge, double max_gain, float *__restrict__ coeffs,
                                                          float *__restrict__ scale, double *__restrict__ sums,
                                                          int *__restrict__ flags)
{
    __shared__ double S[SH_MAX_SUMS];
    __shared__ double A[SH_MAXK][SH_MAXK];
    __shared__ double x[SH_MAXK];
    const ShShape s = sh_shape(order, even);
    const size_t b = blockIdx.x;
    const double *pr = partials + b * (size_t)n_chunks * s.NS;
    for (int i = 0; i < s.NS; ++i) {
        const double v = sh_wave_chunks(pr, n_chunks, s.NS, i);
        if (threadIdx.x == 0) S[i] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    bool bad;
    const float r = sh_scale(S[0], N, bad);
    int flag = bad ? 1 : 0;
    for (int k = 0; k < s.K; ++k) x[k] = S[1 + s.NM + k];
    if (!flag && !sh_cholesky_solve(s, S + 1, ridge, A, x)) flag = 1;
    if (!flag) {
        double l1 = 0.0;
        for (int k = 0; k < s.K; ++k) l1 += fabs((double)(float)x[k]);
        if (!(l1 <= max_gain)) flag = 2;
    }
    for (int k = 0; k < s.K; ++k) coeffs[b * s.K + k] = flag ? (k == 0 ? 1.0f : 0.0f) : (float)x[k];
    scale[b] = r;
    flags[b] = flag;
    for (int i = 0; i < s.NS; ++i) sums[b * s.NS + i] = S[i];
}

// C(t) by Horner from the fp32 coefficients, every operation rounded on its own; z = fl32(r C(t))
template <int P, bool EVEN>
__device__ __forceinline__ float sh_apply_one(float xf, double r, const double (&c)[ShCfg<P, EVEN>::K])
{
    constexpr int K = ShCfg<P, EVEN>::K;
    const double t = (double)xf / r;
    const double s = EVEN ? t : t * t;
    double h = c[K - 1];
#pragma unroll
    for (int k = K - 2; k >= 0; --k) h = c[k] + s * h;
    return (float)(r * (t * h));
}

template <int P, bool EVEN>
__global__ __launch_bounds__(SH_THREADS) void shaper_apply_kernel(const float *__restrict__ y_hat, long long y_hat_stride,
                                                                  const float *__restrict__ coeffs,
                                                                  const float *__restrict__ scale, const int *__restrict__ flags,
                                                                  int N, float *__restrict__ z, long long z_stride)
{
    constexpr int K = ShCfg<P, EVEN>::K;
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * SH_CHUNK;
    const int len = min(SH_CHUNK, N - n0);
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    float *o = z + b * (size_t)z_stride + n0;
    if (flags[b]) {                                                 // the identity: a copy, bit for bit
        sh_walk(o, len, [&](int i) { o[i] = p[i]; },
                [&](int i) {
                    const RowsUFloat4 u = sh_ldu(p + i);
                    *reinterpret_cast<float4 *>(o + i) = make_float4(u.x, u.y, u.z, u.w);
                });
        return;
    }
    const double r = (double)scale[b];
    double c[K];
#pragma unroll
    for (int k = 0; k < K; ++k) c[k] = (double)coeffs[b * K + k];
    sh_walk(o, len, [&](int i) { o[i] = sh_apply_one<P, EVEN>(p[i], r, c); },
            [&](int i) {
                const RowsUFloat4 u = sh_ldu(p + i);
                *reinterpret_cast<float4 *>(o + i) =
                    make_float4(sh_apply_one<P, EVEN>(u.x, r, c), sh_apply_one<P, EVEN>(u.y, r, c),
                                sh_apply_one<P, EVEN>(u.z, r, c), sh_apply_one<P, EVEN>(u.w, r, c));
            });
}

template <int P, bool EVEN>
__device__ __forceinline__ void sh_bwd_sums_one(float df, float xf, double r, double (&g)[ShCfg<P, EVEN>::K])
{
    using C = ShCfg<P, EVEN>;
    const double t = (double)xf / r, d = (double)df;
    double pw = t;
#pragma unroll
    for (int q = 1; q <= P; ++q) {
        if (q > 1) pw = pw * t;
        if (C::is_power(q)) g[C::k_of(q)] = fma(d, pw, g[C::k_of(q)]);
    }
}

template <int P, bool EVEN>
__global__ __launch_bounds__(SH_THREADS) void shaper_bwd_partials_kernel(const float *__restrict__ dz, long long dz_stride,
                                                                         const float *__restrict__ y_hat, long long y_hat_stride,
                                                                         const float *__restrict__ scale, int N,
                                                                         double *__restrict__ partials)
{
    constexpr int K = ShCfg<P, EVEN>::K;
    __shared__ double red[4 * K];
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * SH_CHUNK;
    const int len = min(SH_CHUNK, N - n0);
    const float *d = dz + b * (size_t)dz_stride + n0;
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    const double r = (double)scale[b];
    double g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = 0.0;
    sh_walk(d, len, [&](int i) { sh_bwd_sums_one<P, EVEN>(d[i], p[i], r, g); },
            [&](int i) {
                const float4 u = sh_lda(d + i);
                const RowsUFloat4 w = sh_ldu(p + i);
                sh_bwd_sums_one<P, EVEN>(u.x, w.x, r, g);
                sh_bwd_sums_one<P, EVEN>(u.y, w.y, r, g);
                sh_bwd_sums_one<P, EVEN>(u.z, w.z, r, g);
                sh_bwd_sums_one<P, EVEN>(u.w, w.w, r, g);
            });
    sh_block_sums<K>(g, red);
    if (threadIdx.x == 0) {
        double *o = partials + (b * gridDim.x + blockIdx.x) * (size_t)K;
#pragma unroll
        for (int k = 0; k < K; ++k) o[k] = g[k];
    }
}

__global__ __launch_bounds__(64) void shaper_bwd_solve_kernel(const double *__restrict__ partials, const double *__restrict__ sums,
                                                              const int *__restrict__ flags, int n_chunks, int order, int even,
                                                              double ridge, double *__restrict__ u)
{
    __shared__ double A[SH_MAXK][SH_MAXK];
    __shared__ double x[SH_MAXK];
    const ShShape s = sh_shape(order, even);
    const size_t b = blockIdx.x;
    const double *pr = partials + b * (size_t)n_chunks * s.K;
    for (int k = 0; k < s.K; ++k) {
        const double v = sh_wave_chunks(pr, n_chunks, s.K, k);
        if (threadIdx.x == 0) x[k] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // an unflagged row's pivots were positive in the forward, which ran this very factorisation on these very sums
    const bool ok = !flags[b] && sh_cholesky_solve(s, sums + b * s.NS + 1, ridge, A, x);
    for (int k = 0; k < s.K; ++k) u[b * s.K + k] = ok ? x[k] : 0.0;
}

// one element of the backward in fp64, rounded once.  cp = p_k c_k, up = p_k u_k, w = 2 ridge u_k c_k p_k.
template <int P, bool EVEN>
__device__ __forceinline__ float sh_bwd_one(float df, float xf, float yf, double r, const double (&c)[ShCfg<P, EVEN>::K],
                                            const double (&cp)[ShCfg<P, EVEN>::K], const double (&u)[ShCfg<P, EVEN>::K],
                                            const double (&up)[ShCfg<P, EVEN>::K], const double (&w)[ShCfg<P, EVEN>::K])
{
    using C = ShCfg<P, EVEN>;
    const double t = (double)xf / r, yr = (double)yf / r;
    double pw[2 * P];                                               // t^0 .. t^(2 P - 1)
    pw[0] = 1.0;
#pragma unroll
    for (int q = 1; q < 2 * P; ++q) pw[q] = pw[q - 1] * t;
    double Ct = 0.0, Cd = 0.0, Ut = 0.0, Ud = 0.0, R = 0.0;
#pragma unroll
    for (int k = 0; k < C::K; ++k) {
        const int p = C::power(k);
        Ct += c[k] * pw[p];
        Cd += cp[k] * pw[p - 1];
        Ut += u[k] * pw[p];
        Ud += up[k] * pw[p - 1];
        R += w[k] * pw[2 * p - 1];
    }
    return (float)((((double)df * Cd + Ud * yr) - (Ud * Ct + Ut * Cd)) - R);
}

template <int P, bool EVEN>
__global__ __launch_bounds__(SH_THREADS) void shaper_bwd_apply_kernel(const float *dz, long long dz_stride,
                                                                      const float *__restrict__ y_hat, long long y_hat_stride,
                                                                      const float *__restrict__ y, long long y_stride,
                                                                      const float *__restrict__ coeffs,
                                                                      const float *__restrict__ scale, const double *__restrict__ uu,
                                                                      const int *__restrict__ flags, int N, double ridge,
                                                                      float *dy_hat, long long dy_hat_stride)
{
    using C = ShCfg<P, EVEN>;
    constexpr int K = C::K;
    const size_t b = blockIdx.y;
    const int n0 = (int)blockIdx.x * SH_CHUNK;
    const int len = min(SH_CHUNK, N - n0);
    const float *d = dz + b * (size_t)dz_stride + n0;
    const float *p = y_hat + b * (size_t)y_hat_stride + n0;
    const float *q = y + b * (size_t)y_stride + n0;
    float *o = dy_hat + b * (size_t)dy_hat_stride + n0;
    if (flags[b]) {                                                 // the gradient passes through, bit for bit
        if (o == d) return;
        sh_walk(o, len, [&](int i) { o[i] = d[i]; },
                [&](int i) {
                    const RowsUFloat4 v = sh_ldu(d + i);
                    *reinterpret_cast<float4 *>(o + i) = make_float4(v.x, v.y, v.z, v.w);
                });
        return;
    }
    const double r = (double)scale[b];
    double c[K], cp[K], u[K], up[K], w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double pk = (double)C::power(k);
        c[k] = (double)coeffs[b * K + k];
        u[k] = uu[b * K + k];
        cp[k] = pk * c[k];
        up[k] = pk * u[k];
        w[k] = (2.0 * ridge) * (u[k] * cp[k]);
    }
    sh_walk(o, len, [&](int i) { o[i] = sh_bwd_one<P, EVEN>(d[i], p[i], q[i], r, c, cp, u, up, w); },
            [&](int i) {
                const RowsUFloat4 v = sh_ldu(d + i), x = sh_ldu(p + i), t = sh_ldu(q + i);
                *reinterpret_cast<float4 *>(o + i) = make_float4(
                    sh_bwd_one<P, EVEN>(v.x, x.x, t.x, r, c, cp, u, up, w), sh_bwd_one<P, EVEN>(v.y, x.y, t.y, r, c, cp, u, up, w),
                    sh_bwd_one<P, EVEN>(v.z, x.z, t.z, r, c, cp, u, up, w), sh_bwd_one<P, EVEN>(v.w, x.w, t.w, r, c, cp, u, up, w));
            });
}

// C ABI ---------------------------------------------------------------------------------------
static bool sh_bad_order(int32_t order, int32_t even)
{
    return order < 1 || order > MX_SHAPER_MAX_ORDER || (even != 0 && even != 1);
}

static int sh_check_size(int64_t B, int64_t N)
{
    return (N > MX_SHAPER_MAX_N || B > MX_SHAPER_MAX_ROWS) ? MX_ERR_UNSUPPORTED : MX_OK;
}

static bool sh_bad_ridge(double ridge) { return !(ridge >= 0.0) || !(ridge < 1e300); }

static int64_t sh_n_chunks(int64_t N) { return (N + SH_CHUNK - 1) / SH_CHUNK; }

static dim3 sh_grid(int64_t B, int64_t N) { return dim3((unsigned)sh_n_chunks(N), (unsigned)B); }

// CALL(P, EVEN) with the compile-time pair of a run-time shape
#define SH_DISPATCH(shape, CALL)                                                                   \
    do {                                                                                           \
        if ((shape).even) switch ((shape).P) {                                                     \
            case 1: { CALL(1, true); break; }  case 2: { CALL(2, true); break; }                   \
            case 3: { CALL(3, true); break; }  case 4: { CALL(4, true); break; }                   \
            case 5: { CALL(5, true); break; }  case 6: { CALL(6, true); break; }                   \
            default: { CALL(7, true); break; }                                                     \
        } else switch ((shape).P) {                                                                \
            case 1: { CALL(1, false); break; } case 3: { CALL(3, false); break; }                  \
            case 5: { CALL(5, false); break; } default: { CALL(7, false); break; }                 \
        }                                                                                          \
    } while (0)

MX_EXPORT int mx_shaper_match_partials(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                                       int64_t N, int32_t order, int32_t even, double *partials, void *stream)
{
    if (!partials || rows_check(y_hat, y_hat_stride, B, N) || rows_check(y, y_stride, B, N)) return MX_ERR_ARG;
    if (sh_bad_order(order, even)) return MX_ERR_ARG;
    if (sh_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    const ShShape s = sh_shape(order, even);
    const RowsRange out = rows_flat(partials, B * sh_n_chunks(N) * s.NS, 8);
    if (rows_overlap(out, rows_range(y_hat, y_hat_stride, B, N)) || rows_overlap(out, rows_range(y, y_stride, B, N)))
        return MX_ERR_ARG;
    hipLaunchKernelGGL(shaper_s2_kernel, sh_grid(B, N), dim3(SH_THREADS), 0, (hipStream_t)stream, y_hat, (long long)y_hat_stride,
                       (int)N, s.NS, partials);
#define SH_CALL(P, E)                                                                                                          \
    hipLaunchKernelGGL((shaper_moments_kernel<P, E>), sh_grid(B, N), dim3(SH_THREADS), 0, (hipStream_t)stream, y_hat,           \
                       (long long)y_hat_stride, y, (long long)y_stride, (int)N, partials)
    SH_DISPATCH(s, SH_CALL);
#undef SH_CALL
    return mx_launch_status();
}

MX_EXPORT int mx_shaper_match_solve(const double *partials, int64_t B, int64_t N, int64_t n_chunks, int32_t order, int32_t even,
                                    double ridge, double max_gain, float *coeffs, float *scale, double *sums, int32_t *flags,
                                    void *stream)
{
    if (!partials || !coeffs || !scale || !sums || !flags || B < 1 || N < 1 || n_chunks != sh_n_chunks(N)) return MX_ERR_ARG;
    if (sh_bad_order(order, even)) return MX_ERR_ARG;
    if (sh_bad_ridge(ridge) || !(max_gain >= 1.0) || !(max_gain < 1e300)) return MX_ERR_ARG;
    if (sh_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    const ShShape s = sh_shape(order, even);
    const RowsRange out[4] = {rows_flat(coeffs, B * s.K, 4), rows_flat(scale, B, 4), rows_flat(sums, B * s.NS, 8),
                              rows_flat(flags, B, 4)};
    const RowsRange in[1] = {rows_flat(partials, B * n_chunks * s.NS, 8)};
    if (rows_any_overlap(out, 4, in, 1)) return MX_ERR_ARG;
    hipLaunchKernelGGL(shaper_solve_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, partials, (int)N, (int)n_chunks,
                       (int)order, (int)even, ridge, max_gain, coeffs, scale, sums, (int *)flags);
    return mx_launch_status();
}

MX_EXPORT int mx_shaper_match_apply(const float *y_hat, int64_t y_hat_stride, const float *coeffs, const float *scale,
                                    const int32_t *flags, int64_t B, int64_t N, int32_t order, int32_t even, float *z,
                                    int64_t z_stride, void *stream)
{
    if (!coeffs || !scale || !flags || rows_check(y_hat, y_hat_stride, B, N) || rows_check(z, z_stride, B, N)) return MX_ERR_ARG;
    if (sh_bad_order(order, even)) return MX_ERR_ARG;
    if (sh_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    const ShShape s = sh_shape(order, even);
    const RowsRange out[1] = {rows_range(z, z_stride, B, N)};
    const RowsRange in[4] = {rows_range(y_hat, y_hat_stride, B, N), rows_flat(coeffs, B * s.K, 4), rows_flat(scale, B, 4),
                             rows_flat(flags, B, 4)};
    if (rows_any_overlap(out, 1, in, 4)) return MX_ERR_ARG;
#define SH_CALL(P, E)                                                                                                          \
    hipLaunchKernelGGL((shaper_apply_kernel<P, E>), sh_grid(B, N), dim3(SH_THREADS), 0, (hipStream_t)stream, y_hat,             \
                       (long long)y_hat_stride, coeffs, scale, (const int *)flags, (int)N, z, (long long)z_stride)
    SH_DISPATCH(s, SH_CALL);
#undef SH_CALL
    return mx_launch_status();
}

MX_EXPORT int mx_shaper_match_bwd_partials(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride,
                                           const float *scale, int64_t B, int64_t N, int32_t order, int32_t even,
                                           double *partials, void *stream)
{
    if (!scale || !partials || rows_check(dz, dz_stride, B, N) || rows_check(y_hat, y_hat_stride, B, N)) return MX_ERR_ARG;
    if (sh_bad_order(order, even)) return MX_ERR_ARG;
    if (sh_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    const ShShape s = sh_shape(order, even);
    const RowsRange out[1] = {rows_flat(partials, B * sh_n_chunks(N) * s.K, 8)};
    const RowsRange in[3] = {rows_range(dz, dz_stride, B, N), rows_range(y_hat, y_hat_stride, B, N), rows_flat(scale, B, 4)};
    if (rows_any_overlap(out, 1, in, 3)) return MX_ERR_ARG;
#define SH_CALL(P, E)                                                                                                          \
    hipLaunchKernelGGL((shaper_bwd_partials_kernel<P, E>), sh_grid(B, N), dim3(SH_THREADS), 0, (hipStream_t)stream, dz,         \
                       (long long)dz_stride, y_hat, (long long)y_hat_stride, scale, (int)N, partials)
    SH_DISPATCH(s, SH_CALL);
#undef SH_CALL
    return mx_launch_status();
}

MX_EXPORT int mx_shaper_match_bwd_solve(const double *partials, const double *sums, const int32_t *flags, int64_t B,
                                        int64_t n_chunks, int32_t order, int32_t even, double ridge, double *u, void *stream)
{
    if (!partials || !sums || !flags || !u || B < 1 || n_chunks < 1) return MX_ERR_ARG;
    if (sh_bad_order(order, even)) return MX_ERR_ARG;
    if (sh_bad_ridge(ridge)) return MX_ERR_ARG;
    if (B > MX_SHAPER_MAX_ROWS || n_chunks > sh_n_chunks(MX_SHAPER_MAX_N)) return MX_ERR_UNSUPPORTED;
    const ShShape s = sh_shape(order, even);
    const RowsRange out[1] = {rows_flat(u, B * s.K, 8)};
    const RowsRange in[3] = {rows_flat(partials, B * n_chunks * s.K, 8), rows_flat(sums, B * s.NS, 8), rows_flat(flags, B, 4)};
    if (rows_any_overlap(out, 1, in, 3)) return MX_ERR_ARG;
    hipLaunchKernelGGL(shaper_bwd_solve_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, partials, sums,
                       (const int *)flags, (int)n_chunks, (int)order, (int)even, ridge, u);
    return mx_launch_status();
}

MX_EXPORT int mx_shaper_match_bwd_apply(const float *dz, int64_t dz_stride, const float *y_hat, int64_t y_hat_stride,
                                        const float *y, int64_t y_stride, const float *coeffs, const float *scale, const double *u,
                                        const int32_t *flags, int64_t B, int64_t N, int32_t order, int32_t even, double ridge,
                                        float *dy_hat, int64_t dy_hat_stride, void *stream)
{
    if (!coeffs || !scale || !u || !flags || rows_check(dz, dz_stride, B, N) || rows_check(y_hat, y_hat_stride, B, N)
        || rows_check(y, y_stride, B, N) || rows_check(dy_hat, dy_hat_stride, B, N))
        return MX_ERR_ARG;
    if (sh_bad_order(order, even)) return MX_ERR_ARG;
    if (sh_bad_ridge(ridge)) return MX_ERR_ARG;
    if (sh_check_size(B, N)) return MX_ERR_UNSUPPORTED;
    const ShShape s = sh_shape(order, even);
    const bool in_place = dy_hat == dz && dy_hat_stride == dz_stride;
    const RowsRange out[1] = {rows_range(dy_hat, dy_hat_stride, B, N)};
    const RowsRange in[6] = {rows_range(y_hat, y_hat_stride, B, N), rows_range(y, y_stride, B, N), rows_flat(coeffs, B * s.K, 4),
                             rows_flat(scale, B, 4), rows_flat(u, B * s.K, 8), rows_flat(flags, B, 4)};
    if ((!in_place && rows_overlap(out[0], rows_range(dz, dz_stride, B, N))) || rows_any_overlap(out, 1, in, 6)) return MX_ERR_ARG;
#define SH_CALL(P, E)                                                                                                          \
    hipLaunchKernelGGL((shaper_bwd_apply_kernel<P, E>), sh_grid(B, N), dim3(SH_THREADS), 0, (hipStream_t)stream, dz,            \
                       (long long)dz_stride, y_hat, (long long)y_hat_stride, y, (long long)y_stride, coeffs, scale, u,          \
                       (const int *)flags, (int)N, ridge, dy_hat, (long long)dy_hat_stride)
    SH_DISPATCH(s, SH_CALL);
#undef SH_CALL
    return mx_launch_status();
}
