// lfo_stitch.hip -- K22: one LFO track along a whole recording from the LFOs of overlapping windows -- no counterpart in
// the reference (include/modex_hip.h, K22, has the definition).
//
//     p_j = j (L - 1) / (n_t - 1);   over the windows with s_w <= p_j <= s_w + N - 1, ascending w:
//     track[j] = sum_w a_w v_w / sum_w a_w,   v_w = window w interpolated linearly at p_j,   a_w = sin^2(pi u) + 1e-3
//
// One thread per track point, grid over tiles of LS_THREADS points.  j (L - 1) is an exact fp64 integer (the launcher's
// limits), so p_j is one correctly rounded division and its comparisons with integers are exact.  The starts are
// ascending, so "s_w + N - 1 >= p_j" is monotone in w: the first such window comes from a binary search (<= 20 loads of an
// L2-resident list), and the walk from it ends at the first s_w > p_j.  An index into a window is clamped to its row
// whatever the starts hold, so no list can make the kernel read outside `windows`.  No atomics, no workspace, no LDS.
// A 60 s recording is some 10^4 points and a few hundred windows: launch latency; there is nothing here to tune.
#include "rows_common.h"

#define LS_THREADS 256
#define LS_MAX_L (1ll << 31)
#define LS_MAX_POINTS (1ll << 22)

__global__ __launch_bounds__(LS_THREADS) void lfo_stitch_kernel(
    const float *__restrict__ windows, const long long *__restrict__ starts, int W, int n_f, long long N, long long L, int n_t,
    float *__restrict__ track, int *__restrict__ cover)
{
    const int j = (int)(blockIdx.x * LS_THREADS + threadIdx.x);
    if (j >= n_t) return;
    const double p = (double)((long long)j * (L - 1)) / (double)(n_t - 1);
    const double last = (double)(N - 1);
    int lo = 0, hi = W;                                             // the first w with s_w + N - 1 >= p, or W
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)starts[mid] + last >= p) hi = mid; else lo = mid + 1;
    }
    const double to_frame = (double)(n_f - 1) / last;
    double num = 0.0, den = 0.0;
    int count = 0;
    for (int w = lo; w < W; ++w) {
        const double s = (double)starts[w];
        if (s > p) break;
        if (s + last < p) continue;                                 // only an unsorted list gets here
        const double rel = p - s;
        const double t = rel * to_frame;
        int i0 = (int)floor(t);
        i0 = i0 < 0 ? 0 : (i0 > n_f - 2 ? n_f - 2 : i0);
        const float *x = windows + (size_t)w * (size_t)n_f + i0;
        const double x0 = (double)x[0], x1 = (double)x[1];
        const double f = t - (double)i0;
        const double v = (1.0 - f) * x0 + f * x1;
        const double sn = sinpi((rel + 0.5) / (double)N);
        const double a = sn * sn + 1e-3;
        num += a * v;
        den += a;
        ++count;
    }
    track[j] = count ? (float)(num / den) : 0.0f;
    cover[j] = count;
}

// C ABI ---------------------------------------------------------------------------------------
MX_EXPORT int mx_lfo_stitch(const float *windows, const int64_t *starts, int64_t W, int64_t n_f, int64_t N, int64_t L,
                            int64_t n_t, float *track, int32_t *cover, void *stream)
{
    if (!windows || !starts || !track || !cover) return MX_ERR_ARG;
    if (W < 1 || n_f < 2 || N < 2 || L < N || n_t < 2) return MX_ERR_ARG;
    if (W > MX_STITCH_MAX_WINDOWS || L > LS_MAX_L || n_f > LS_MAX_POINTS || n_t > LS_MAX_POINTS) return MX_ERR_UNSUPPORTED;
    const RowsRange out[2] = {rows_flat(track, n_t, 4), rows_flat(cover, n_t, 4)};
    const RowsRange in[2] = {rows_flat(windows, W * n_f, 4), rows_flat(starts, W, 8)};
    if (rows_any_overlap(out, 2, in, 2)) return MX_ERR_ARG;
    const unsigned grid = (unsigned)((n_t + LS_THREADS - 1) / LS_THREADS);
    hipLaunchKernelGGL(lfo_stitch_kernel, dim3(grid), dim3(LS_THREADS), 0, (hipStream_t)stream, windows,
                       (const long long *)starts, (int)W, (int)n_f, (long long)N, (long long)L, (int)n_t, track, (int *)cover);
    return mx_launch_status();
}
