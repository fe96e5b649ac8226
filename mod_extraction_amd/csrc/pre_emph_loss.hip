// pre_emph_loss.hip -- K15: the FIR pre-emphasis of mod_extraction/wright_code.py:47-73 (WrightPreEmph) and the ESR of
// losses.py:34-38 taken after it, as value and gradient.
//
// The linear map F on a row x[0..T), the two stages applied one after the other in fp32 as the reference does:
//   stage 1  f[n] = sum_k c[k] x[n-(K-1)+k]     n = 0..T-1, x[<0] = 0   (K-1 zeros in front, Conv1d = cross-correlation)
//   stage 2  g[n] = 0.85 f[n] + f[n+1]          n = 0..T-2              (only with low_pass: no padding, one sample shorter)
// so F x has L = T (no low_pass) or T - 1 entries.  F^T is the exact transpose, boundary rows included:
//   stage 2^T  h[m] = 0.85 g[m] + g[m-1]        m = 0..T-1, g[<0] = g[>=L] = 0
//   stage 1^T  x'[j] = sum_k c[k] h[j+(K-1)-k]  j = 0..T-1, h[>=T] = 0
//
// All kernels work on tiles of PE_TILE samples staged through two LDS buffers that ping-pong between the stages.  Both
// buffers share one layout: entry i holds sample m = base + i with base = t0 - 1 - H (H = K - 1), nb = nq + 2 H + 2 entries
// for a tile of nq = min(PE_TILE, T - t0) samples, which is the widest halo any stage needs: the outputs j in [t0, t0 + nq)
// of F^T F read h up to j + H, h reads g one behind, g reads f one ahead, f reads x up to H behind.  Every stage writes 0
// where its sample lies outside the row, so the row ends and the T - 1 tail need no special case downstream.  A workgroup
// walks its row tile by tile and every tile is a chain load -> barrier -> stage -> barrier -> ...: the tile is large (16 loads
// in flight per thread) so that a 2 s clip is 22 such chains, not 87.
#include "common.h"

#define PE_TILE 4096
#define PE_MAXK 16
#define PE_NB (PE_TILE + 2 * (PE_MAXK - 1) + 2)
#define PE_LP0 0.85f                 // wright_code.py:59: the low-pass taps [0.85, 1]

// f[i], i in [H, nb): stage 1 from d[i-H .. i]
__device__ __forceinline__ void pe_stage1(const float *d, float *f, const float *c, int K, int base, int T, int nb)
{
    const int H = K - 1;
    for (int i = H + (int)threadIdx.x; i < nb; i += 256) {
        const int m = base + i;
        float s = 0.0f;
        if (m >= 0 && m < T) {
            s = c[0] * d[i - H];
            for (int k = 1; k < K; ++k) s += c[k] * d[i - H + k];
        }
        f[i] = s;
    }
}

// g[i], i in [lo, hi): stage 2 from f[i], f[i+1]; g = 0 outside [0, L)
__device__ __forceinline__ void pe_stage2(const float *f, float *g, int lo, int hi, int base, int L)
{
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const int m = base + i;
        g[i] = (m >= 0 && m < L) ? PE_LP0 * f[i] + f[i + 1] : 0.0f;
    }
}

// h[i], i in [lo, hi): stage 2 transposed from g[i], g[i-1] (g is 0 outside [0, L)); h = 0 outside [0, T)
__device__ __forceinline__ void pe_stage2t(const float *g, float *h, int lo, int hi, int base, int T)
{
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const int m = base + i;
        h[i] = (m >= 0 && m < T) ? PE_LP0 * g[i] + g[i - 1] : 0.0f;
    }
}

// stage 1 transposed for output sample j = t0 + q: reads h[q+H+1 .. q+2H+1] (h is 0 at and beyond T)
__device__ __forceinline__ float pe_stage1t(const float *h, const float *c, int K, int q)
{
    const int H = K - 1, i = q + H + 1;
    float s = c[0] * h[i + H];
    for (int k = 1; k < K; ++k) s += c[k] * h[i + H - k];
    return s;
}

// F of the tile whose samples (zero outside the row) fill bufA: returns the buffer that holds F (entries [H, nb - 1) are
// valid; 0 outside [0, L)).  Called by all 256 threads; the result is visible to all on return.
__device__ __forceinline__ float *pe_filter_tile(float *bufA, float *bufB, const float *c, int K, int low_pass, int base,
                                                 int T, int L, int nb)
{
    __syncthreads();
    pe_stage1(bufA, bufB, c, K, base, T, nb);
    __syncthreads();
    if (!low_pass) return bufB;
    pe_stage2(bufB, bufA, K - 1, nb - 1, base, L);
    __syncthreads();
    return bufA;
}

// bufA[i] = a[m] - t[m] (t == nullptr: a[m]) for the samples m = base + i inside [0, n), else 0
__device__ __forceinline__ void pe_load_tile(float *bufA, const float *a, const float *t, int base, int n, int nb)
{
    __syncthreads();                                            // the previous tile may still be read
    for (int i = threadIdx.x; i < nb; i += 256) {
        const int m = base + i;
        float v = 0.0f;
        if (m >= 0 && m < n) v = t ? a[m] - t[m] : a[m];
        bufA[i] = v;
    }
}

// sum over the tile's own samples [t0, t0 + nq) inside [0, L) of r^2, fp64
__device__ __forceinline__ double pe_tile_sumsq(const float *r, int K, int t0, int nq, int L)
{
    double s = 0.0;
    for (int q = threadIdx.x; q < nq; q += 256)
        if (t0 + q < L) {
            const double v = (double)r[q + K];
            s += v * v;
        }
    return s;
}

// per-row sums ( sum (F(a - t))^2, sum (F t)^2 ): fp64, fixed order (tiles in order per thread, then lanes, then waves)
__device__ __forceinline__ void pe_row_sums(const float *a, const float *t, int T, int L, const float *c, int K,
                                            int low_pass, float *bufA, float *bufB, double *red, double &s_ee, double &s_yy)
{
    const int H = K - 1;
    s_ee = 0.0; s_yy = 0.0;
    for (int t0 = 0; t0 < L; t0 += PE_TILE) {
        const int base = t0 - 1 - H, nq = min(PE_TILE, T - t0), nb = nq + 2 * H + 2;
        pe_load_tile(bufA, a, t, base, T, nb);
        s_ee += pe_tile_sumsq(pe_filter_tile(bufA, bufB, c, K, low_pass, base, T, L, nb), K, t0, nq, L);
        pe_load_tile(bufA, t, nullptr, base, T, nb);
        s_yy += pe_tile_sumsq(pe_filter_tile(bufA, bufB, c, K, low_pass, base, T, L, nb), K, t0, nq, L);
    }
    s_ee = block256_sum_f64(s_ee, red);
    s_yy = block256_sum_f64(s_yy, red);
}

__device__ __forceinline__ void pe_load_taps(float *c, const float *taps, int K)
{
    if ((int)threadIdx.x < PE_MAXK) c[threadIdx.x] = (int)threadIdx.x < K ? taps[threadIdx.x] : 0.0f;
    __syncthreads();
}


// out[b, 0..L) = F(x[b, 0..T))   or, transposed,   out[b, 0..T) = F^T(x[b, 0..L)).  grid (tiles, B).
__global__ __launch_bounds__(256) void pre_emph_kernel(const float *__restrict__ x, long long xs, int T, int L,
                                                       const float *__restrict__ taps, int K, int low_pass, int transpose,
                                                       float *__restrict__ out, long long os)
{
    __shared__ float bufA[PE_NB], bufB[PE_NB], c[PE_MAXK];
    pe_load_taps(c, taps, K);
    const float *xr = x + (size_t)blockIdx.y * xs;
    float *o = out + (size_t)blockIdx.y * os;
    const int H = K - 1, t0 = blockIdx.x * PE_TILE, base = t0 - 1 - H, nq = min(PE_TILE, T - t0), nb = nq + 2 * H + 2;
    if (!transpose) {
        pe_load_tile(bufA, xr, nullptr, base, T, nb);
        const float *r = pe_filter_tile(bufA, bufB, c, K, low_pass, base, T, L, nb);
        for (int q = threadIdx.x; q < nq; q += 256)
            if (t0 + q < L) o[t0 + q] = r[q + K];
    } else {
        pe_load_tile(bufA, xr, nullptr, base, L, nb);
        __syncthreads();
        const float *h = bufA;                                  // no low_pass: L == T and stage 2^T is the identity
        if (low_pass) {
            pe_stage2t(bufA, bufB, 1, nb, base, T);
            __syncthreads();
            h = bufB;
        }
        for (int q = threadIdx.x; q < nq; q += 256) o[t0 + q] = pe_stage1t(h, c, K, q);
    }
}

// x: B rows of T samples (transpose != 0: of L samples); out: B rows of L samples (transpose != 0: of T samples).
MX_EXPORT int mx_pre_emph(const float *x, int64_t x_stride, int64_t B, int64_t T, const float *taps, int64_t K,
                          int32_t low_pass, int32_t transpose, float *out, int64_t out_stride, void *stream)
{
    const int64_t L = low_pass ? T - 1 : T;
    if (!x || !taps || !out || B <= 0 || T <= 0 || L <= 0) return MX_ERR_ARG;
    if (x_stride < (transpose ? L : T) || out_stride < (transpose ? T : L)) return MX_ERR_ARG;
    if (K < 1 || K > PE_MAXK || T >= (1ll << 30) || B > 65535) return MX_ERR_UNSUPPORTED;
    const int64_t n_out = transpose ? T : L;
    hipLaunchKernelGGL(pre_emph_kernel, dim3((unsigned)((n_out + PE_TILE - 1) / PE_TILE), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, x, (long long)x_stride, (int)T, (int)L, taps, (int)K, (int)(low_pass != 0),
                       (int)(transpose != 0), out, (long long)out_stride);
    return mx_launch_status();
}


// One workgroup per row: the reduction sweep of pe_row_sums; with dy != nullptr the write sweep follows while the row is
// cache-resident:  dy (+)= (2 w / B) F^T F (y_hat - y) / (sum (F y)^2 + eps).
__global__ __launch_bounds__(256) void pre_emph_esr_kernel(const float *__restrict__ y_hat, long long hs,
                                                           const float *__restrict__ y, long long ys, int B, int T, int L,
                                                           const float *__restrict__ taps, int K, int low_pass, float w,
                                                           float eps, int accumulate, float *__restrict__ part,
                                                           float *__restrict__ dy, long long ds)
{
    __shared__ float bufA[PE_NB], bufB[PE_NB], c[PE_MAXK];
    __shared__ double red[4];
    pe_load_taps(c, taps, K);
    const int b = blockIdx.x;
    const float *a = y_hat + (size_t)b * hs, *t = y + (size_t)b * ys;
    double s_ee, s_yy;
    pe_row_sums(a, t, T, L, c, K, low_pass, bufA, bufB, red, s_ee, s_yy);
    if (threadIdx.x == 0) {
        part[(size_t)b * 2] = (float)s_ee;
        part[(size_t)b * 2 + 1] = (float)s_yy;
    }
    if (!dy) return;
    float *o = dy + (size_t)b * ds;
    const float coef = (float)(2.0 * (double)w / (double)B / (s_yy + (double)eps));
    const int H = K - 1;
    for (int t0 = 0; t0 < T; t0 += PE_TILE) {
        const int base = t0 - 1 - H, nq = min(PE_TILE, T - t0), nb = nq + 2 * H + 2;
        pe_load_tile(bufA, a, t, base, T, nb);
        const float *h = pe_filter_tile(bufA, bufB, c, K, low_pass, base, T, L, nb);
        if (low_pass) {                                         // F is in bufA, entries [H, nb - 1)
            pe_stage2t(bufA, bufB, H + 1, nb - 1, base, T);
            __syncthreads();
            h = bufB;
        }
        for (int q = threadIdx.x; q < nq; q += 256) {
            // the product keeps its own rounding (no FMA with the add below, whatever the contraction flags): what is
            // accumulated is bit for bit the gradient an accumulate = 0 launch writes, dy = fl(dy + p)
            const float g = __fmul_rn(coef, pe_stage1t(h, c, K, q));
            o[t0 + q] = accumulate ? __fadd_rn(o[t0 + q], g) : g;
        }
    }
}

static int pe_esr_check(const float *y_hat, const float *y, const float *taps, const float *part, int64_t B, int64_t T,
                        int64_t K, int32_t low_pass)
{
    if (!y_hat || !y || !taps || !part || B <= 0 || T <= 0 || (low_pass ? T - 1 : T) <= 0) return MX_ERR_ARG;
    if (K < 1 || K > PE_MAXK || T >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    return MX_OK;
}

// y_hat, y: B rows of T samples with row strides; part (B, 2) = ( sum (F(y - y_hat))^2, sum (F y)^2 ).
MX_EXPORT int mx_pre_emph_esr_sums(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                                   int64_t T, const float *taps, int64_t K, int32_t low_pass, float *part, void *stream)
{
    const int rc = pe_esr_check(y_hat, y, taps, part, B, T, K, low_pass);
    if (rc != MX_OK) return rc;
    hipLaunchKernelGGL(pre_emph_esr_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, y_hat,
                       (long long)y_hat_stride, y, (long long)y_stride, (int)B, (int)T, (int)(low_pass ? T - 1 : T), taps,
                       (int)K, (int)(low_pass != 0), 0.0f, 0.0f, 0, part, (float *)nullptr, 0ll);
    return mx_launch_status();
}

// dy (B rows of T samples, stride dy_stride) = or += w * d/d y_hat [ mean_b sum (F(y - y_hat))^2 / (sum (F y)^2 + eps) ];
// part as mx_pre_emph_esr_sums leaves it.
MX_EXPORT int mx_pre_emph_esr_grad(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                                   int64_t T, const float *taps, int64_t K, int32_t low_pass, float w, float eps,
                                   int32_t accumulate, float *part, float *dy, int64_t dy_stride, void *stream)
{
    if (!dy || dy_stride < T) return MX_ERR_ARG;
    const int rc = pe_esr_check(y_hat, y, taps, part, B, T, K, low_pass);
    if (rc != MX_OK) return rc;
    hipLaunchKernelGGL(pre_emph_esr_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, y_hat,
                       (long long)y_hat_stride, y, (long long)y_stride, (int)B, (int)T, (int)(low_pass ? T - 1 : T), taps,
                       (int)K, (int)(low_pass != 0), w, eps, (int)(accumulate != 0), part, dy, (long long)dy_stride);
    return mx_launch_status();
}
