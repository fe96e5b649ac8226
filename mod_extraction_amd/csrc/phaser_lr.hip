// phaser_lr.hip -- K3c: the phaser's LFO at a low rate (the reference has no counterpart: its phaser is pedalboard's, on
// the CPU, with a built-in oscillator and no gradient).
//
// The scan (phaser.hip) and its adjoint (phaser_bwd.hip) take the external LFO on the cut-off-update grid: one value per 4
// source samples, counted from the start of the source row, lead-in included.  An extractor predicts n_mod points over the N
// samples of the clip window.  The two kernels here are the linear map between the two grids and its transpose:
//
//   expand   mod_g[b, g] = m_b(clamp(4 g - lead[b], 0, N - 1))  for g < ceil((lead[b] + N) / 4),  0.5 beyond (the value the
//            scan substitutes for a group it has no LFO for), where m_b(n) is the low-rate row resampled at sample n with
//            interp_tap / interp_combine (common.h) and the scale of interp_scale_host -- the definition of the flanger's
//            fl_lfo and the tremolo's tr_mod: held at its first value through the lead-in, a plain read for n_mod == N.
//            One thread per group, coalesced stores.
//   gather   dmod_lr[b, k] = sum_g w(g, k) dmod_g[b, g]: one wave per (row, point).  The groups that have a tap on point k
//            form one contiguous range (the sample a group reads does not decrease with g, nor does its i0); its first
//            group comes from an estimate that is corrected with the forward's own taps, as tremolo.hip pass 2 does.  The
//            weights are interp_tap's fp32 taps, products and sums fp64 in a fixed order (per lane, then a butterfly),
//            rounded to fp32 once.  No atomics, no (B, N) workspace: two runs are bit-identical.
//
// Both kernels take an optional row list (mx_phaser_mod_expand_rows / mx_phaser_dmod_gather_rows): the grid then covers
// n_rows x tiles and a workgroup works on row b = rows[blockIdx.x / tiles] of the FULL batch -- every buffer stays indexed by
// b, rows that are not listed are neither read nor written, and a listed row goes through the very same code as without a
// list, so its result has the same bits.  That lets the phaser rows of a batch of mixed effects write into buffers they share
// with the other effects' rows.
#include "common.h"

#define PL_THREADS 256
#define PL_WAVES (PL_THREADS / 64)

// the clip sample group g of a row with `lead` lead-in samples takes its LFO from
__device__ __forceinline__ int pl_sample(int g, int lead, int N)
{
    return (int)min(max(4ll * g - lead, 0ll), (long long)N - 1);       // 64-bit: lead is device data
}
// its taps on the low-rate row; n_mod == N: the row itself
__device__ __forceinline__ InterpTap pl_tap(float scale, int n, int n_mod, bool full)
{
    if (!full) return interp_tap(scale, n, n_mod);
    InterpTap t;
    t.i0 = t.i1 = n;
    t.lam0 = 1.0f;
    t.lam1 = 0.0f;
    return t;
}
// groups of row b that carry the LFO: ceil((lead + N) / 4), at most the n_groups the buffer holds
__device__ __forceinline__ int pl_groups(int lead, int N, int n_groups)
{
    const long long t = (long long)lead + N;
    return t <= 0 ? 0 : (int)min((t + 3) / 4, (long long)n_groups);
}

__global__ __launch_bounds__(PL_THREADS) void phaser_mod_expand_kernel(
    const float *__restrict__ mod_lr, int n_mod, float scale, const int *__restrict__ lead, const int *__restrict__ rows,
    int B, int N, int n_groups, int tiles, float *__restrict__ mod_g, long long mod_g_stride)
{
    const int item = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int b = rows ? rows[item] : item;
    const int g = tile * PL_THREADS + (int)threadIdx.x;
    if (g >= n_groups || (unsigned)b >= (unsigned)B) return;          // a listed index outside the batch: nothing is touched
    const int ld = lead ? lead[b] : 0;
    const float *row = mod_lr + (size_t)b * n_mod;
    float v = 0.5f;
    if (g < pl_groups(ld, N, n_groups)) {
        const int n = pl_sample(g, ld, N);
        if (n_mod == N) {
            v = row[n];
        } else {
            const InterpTap t = interp_tap(scale, n, n_mod);
            v = interp_combine(t, row[t.i0], row[t.i1]);
        }
    }
    mod_g[(size_t)b * mod_g_stride + g] = v;
}

__global__ __launch_bounds__(PL_THREADS) void phaser_dmod_gather_kernel(
    const float *__restrict__ dmod_g, long long dmod_g_stride, int n_groups, const int *__restrict__ lead,
    const int *__restrict__ rows, int B, int N, int n_mod, float scale, int tiles, float *__restrict__ dmod_lr)
{
    const int item = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int b = rows ? rows[item] : item;                           // the same for the whole workgroup
    const int lane = threadIdx.x & 63;
    const int k = tile * PL_WAVES + (int)(threadIdx.x >> 6);
    // whole waves leave (k is one per wave, b one per workgroup): the butterfly below stays full
    if (k >= n_mod || (unsigned)b >= (unsigned)B) return;
    const int ld = lead ? lead[b] : 0;
    const int G = pl_groups(ld, N, n_groups);
    const float *gb = dmod_g + (size_t)b * dmod_g_stride;
    const bool full = n_mod == N;
    // point k is tap i0 of the groups with i0 == k and tap i1 of those with i0 == k - 1.  k <= 1: the range starts at group
    // 0 (every lead-in group reads sample 0, whose i0 is 0).  k > 1: an estimate of the first group with i0 >= k - 1 (its
    // sample is > 0, so it lies behind the lead-in), corrected with the forward's own taps.
    int g0 = 0;
    if (k > 1) {
        const int n_est = full ? k - 1 : (int)fminf((float)(k - 1) / scale, (float)(N - 1));
        g0 = (int)min(max(((long long)n_est + ld) >> 2, 0ll), (long long)G);
        while (g0 > 0 && pl_tap(scale, pl_sample(g0 - 1, ld, N), n_mod, full).i0 >= k - 1) --g0;
        while (g0 < G && pl_tap(scale, pl_sample(g0, ld, N), n_mod, full).i0 < k - 1) ++g0;
    }
    double acc = 0.0;
    for (int g = g0 + lane; g < G; g += 64) {
        const InterpTap t = pl_tap(scale, pl_sample(g, ld, N), n_mod, full);
        if (t.i0 > k) break;
        const double wgt = (t.i0 == k ? (double)t.lam0 : 0.0) + (t.i1 == k ? (double)t.lam1 : 0.0);
        acc += wgt * (double)gb[g];
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) dmod_lr[(size_t)b * n_mod + k] = (float)acc;
}

// C ABI ---------------------------------------------------------------------------------------
// rows: NULL (all B rows, grid B x tiles) or n_rows indices on the device (grid n_rows x tiles)
static int pl_launch_expand(const float *mod_lr, int64_t n_mod, const int32_t *lead, const int32_t *rows, int64_t n_rows,
                            int64_t B, int64_t N, int64_t x_width, float *mod_g, int64_t mod_g_stride, void *stream)
{
    if (!mod_lr || !mod_g || B <= 0 || N <= 0 || n_mod < 1 || n_mod > N || x_width < N) return MX_ERR_ARG;
    if (x_width >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    const int64_t n_groups = (x_width + 3) / 4;
    if (mod_g_stride < n_groups) return MX_ERR_ARG;
    const int64_t tiles = (n_groups + PL_THREADS - 1) / PL_THREADS, items = rows ? n_rows : B;
    if (B >= (1ll << 31) || items * tiles >= (1ll << 31)) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(phaser_mod_expand_kernel, dim3((unsigned)(items * tiles)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                       mod_lr, (int)n_mod, interp_scale_host(n_mod, N), lead, rows, (int)B, (int)N, (int)n_groups,
                       (int)tiles, mod_g, (long long)mod_g_stride);
    return mx_launch_status();
}

static int pl_launch_gather(const float *dmod_g, int64_t dmod_g_stride, int64_t n_groups, const int32_t *lead,
                            const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, int64_t n_mod, float *dmod_lr,
                            void *stream)
{
    if (!dmod_g || !dmod_lr || B <= 0 || N <= 0 || n_mod < 1 || n_mod > N) return MX_ERR_ARG;
    if (n_groups < (N + 3) / 4 || dmod_g_stride < n_groups) return MX_ERR_ARG;
    if (n_groups >= (1ll << 28)) return MX_ERR_UNSUPPORTED;
    const int64_t tiles = (n_mod + PL_WAVES - 1) / PL_WAVES, items = rows ? n_rows : B;
    if (B >= (1ll << 31) || items * tiles >= (1ll << 31)) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(phaser_dmod_gather_kernel, dim3((unsigned)(items * tiles)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                       dmod_g, (long long)dmod_g_stride, (int)n_groups, lead, rows, (int)B, (int)N, (int)n_mod,
                       interp_scale_host(n_mod, N), (int)tiles, dmod_lr);
    return mx_launch_status();
}

// mod_lr (B, n_mod) fp32 dense, 1 <= n_mod <= N, spanning the N samples of the clip window (align_corners=True); lead (B,)
// int32 lead-in samples of every row, or NULL for 0; x_width: valid floats of a source row (>= N), as given to
// mx_phaser_fwd_stash.  Output mod_g: row b at mod_g + b*mod_g_stride, ceil(x_width / 4) floats, ALL written (0.5 beyond the
// groups of lead[b] + N samples): the `mod` argument of mx_phaser_fwd_stash with n_mod = mod_g_stride.
MX_EXPORT int mx_phaser_mod_expand(const float *mod_lr, int64_t n_mod, const int32_t *lead, int64_t B, int64_t N,
                                   int64_t x_width, float *mod_g, int64_t mod_g_stride, void *stream)
{
    return pl_launch_expand(mod_lr, n_mod, lead, nullptr, 0, B, N, x_width, mod_g, mod_g_stride, stream);
}

// The transpose of mx_phaser_mod_expand.  dmod_g: row b at dmod_g + b*dmod_g_stride, n_groups valid floats as mx_phaser_bwd
// wrote them (its dmod, dmod_stride, n_mod; n_groups >= ceil(N / 4)); lead, N, n_mod as given to the expand.  Output dmod_lr
// (B, n_mod) fp32 dense, every point written.
MX_EXPORT int mx_phaser_dmod_gather(const float *dmod_g, int64_t dmod_g_stride, int64_t n_groups, const int32_t *lead,
                                    int64_t B, int64_t N, int64_t n_mod, float *dmod_lr, void *stream)
{
    return pl_launch_gather(dmod_g, dmod_g_stride, n_groups, lead, nullptr, 0, B, N, n_mod, dmod_lr, stream);
}

// mx_phaser_mod_expand on the n_rows rows listed in rows (device int32, 1 <= n_rows <= B; the indices themselves are device
// data and are not checked here: one outside 0 .. B - 1 is skipped by the kernel).  mod_lr, lead and mod_g are the full
// batch's: a listed row b reads mod_lr + b*n_mod and lead[b] and writes mod_g + b*mod_g_stride, with the bits of the un-listed
// launch; the other rows are neither read nor written.
MX_EXPORT int mx_phaser_mod_expand_rows(const float *mod_lr, int64_t n_mod, const int32_t *lead, const int32_t *rows,
                                        int64_t n_rows, int64_t B, int64_t N, int64_t x_width, float *mod_g,
                                        int64_t mod_g_stride, void *stream)
{
    if (!rows || n_rows < 1 || n_rows > B) return MX_ERR_ARG;
    return pl_launch_expand(mod_lr, n_mod, lead, rows, n_rows, B, N, x_width, mod_g, mod_g_stride, stream);
}

// mx_phaser_dmod_gather on the listed rows, same contract: row b of dmod_lr (B, n_mod) is written for every listed b, the
// others keep what they held (e.g. the gradient rows of the other effects of a mixed batch).
MX_EXPORT int mx_phaser_dmod_gather_rows(const float *dmod_g, int64_t dmod_g_stride, int64_t n_groups, const int32_t *lead,
                                         const int32_t *rows, int64_t n_rows, int64_t B, int64_t N, int64_t n_mod,
                                         float *dmod_lr, void *stream)
{
    if (!rows || n_rows < 1 || n_rows > B) return MX_ERR_ARG;
    return pl_launch_gather(dmod_g, dmod_g_stride, n_groups, lead, rows, n_rows, B, N, n_mod, dmod_lr, stream);
}
