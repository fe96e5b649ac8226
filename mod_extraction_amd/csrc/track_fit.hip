// track_fit.hip -- K23: the LFO fit of lfo_fit.hip (K18; its header comment has the definition) for rows and grids of any
// length -- no counterpart in the reference.  K18 keeps a row in the LDS of ONE workgroup that walks all K J candidates of a
// shape itself: n <= 4096, K <= 512.  K grows with n (df = sr / (rate_div n)), so a long row has tens of thousands of
// candidates a shape: the parallelism is taken from the candidates, and a row's sums are never split.
//
// Workspace (track_fit_abi.h has the size): per (row, shape, candidate tile) one FitBest; per row the centred fp64 row yc,
// (mean, Syy), and per (row, shape) the refined (R, f, phic).  Four launches per TRACK_MAX_ROWS rows:
// track_prep_kernel    one 1024-thread workgroup per row: mean, Syy and yc, in K18's order (lanes by butterfly, then the 16
//     waves in order), so the three have K18's bits.
// track_coarse_kernel  grid (candidate tile, shape, row), 256 threads, one candidate a lane (shape uniform over the workgroup,
//     each its own instantiation, so lfo_value folds to one branch).  yc is staged through LDS MX_TRACK_FIT_ROW_TILE points at a
//     time (16 KB: eight workgroups a CU); every lane reads the same yc[i], a broadcast; the three fp64 accumulators of a
//     candidate run in ascending i with fma, as K18's do at nsub == 1.  The workgroup's (R, c) argmin under fit_less goes to
//     the workspace.  Compute-bound: n template evaluations (a cosf or an fmodf each) a lane.
// track_refine_kernel  one 1024-thread workgroup per (shape, row): the argmin over the tiles' partials under fit_less (a total
//     order: the result does not depend on how they are visited), then rounds 1..L through K18's fit_stage (25 candidates, 32
//     lanes each striding the row, which L2 now holds), accepted only when strictly smaller.
// track_final_kernel   one wave per row: the argmin over the allowed shapes, ties to the lowest id; amp, offset, resid and the
//     per-shape table as K18's wave 0 writes them; the constant-row rule.
// No atomics; a word of the workspace is read only after an earlier launch of the same call wrote it (masked shapes and
// constant rows are skipped by the writer and the reader alike).
#include "lfo_fit_common.h"
#include "track_fit_abi.h"

#define TRACK_TILE_THREADS MX_TRACK_FIT_CAND_TILE
#define TRACK_TILE_WAVES (TRACK_TILE_THREADS / MX_WAVE)
#define TRACK_MAX_ROWS 65535                                    // grid.z of the coarse launch, grid.y of the refinement

__global__ __launch_bounds__(FIT_THREADS) void track_prep_kernel(const float *__restrict__ y, long long y_stride, long long b0,
                                                                 int n, double *__restrict__ stats, double *__restrict__ yc_all)
{
    __shared__ double redd[FIT_WAVES];
    const size_t b = (size_t)b0 + blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & (MX_WAVE - 1), wave = tid / MX_WAVE;
    const float *row = y + b * (size_t)y_stride;
    double *yc = yc_all + b * (size_t)n;

    double s = 0.0;
    for (int i = tid; i < n; i += FIT_THREADS) s += (double)row[i];
    s = wave_sum_f64(s);
    if (lane == 0) redd[wave] = s;
    __syncthreads();
    s = 0.0;
    for (int w = 0; w < FIT_WAVES; ++w) s += redd[w];
    const double mean = s / (double)n;
    double q = 0.0;
    for (int i = tid; i < n; i += FIT_THREADS) {
        const double v = (double)row[i] - mean;
        yc[i] = v;
        q = fma(v, v, q);
    }
    q = wave_sum_f64(q);
    __syncthreads();                                            // redd was read above
    if (lane == 0) redd[wave] = q;
    __syncthreads();
    if (tid != 0) return;
    double Syy = 0.0;
    for (int w = 0; w < FIT_WAVES; ++w) Syy += redd[w];
    stats[2 * b] = mean;
    stats[2 * b + 1] = Syy;
}

// the coarse candidates tile * 256 .. + 255 of shape SH: their (R, c) argmin, returned to thread 0
template <int SH>
__device__ __forceinline__ FitBest track_coarse_tile(const double *__restrict__ yc, int n, float sr, double Syy, double f_min,
                                                     double f_max, double df, int J, long long ncand, double *tile, FitBest *red)
{
    const int tid = (int)threadIdx.x;
    const long long g = (long long)blockIdx.x * TRACK_TILE_THREADS + tid;
    const bool active = g < ncand;
    const int c = active ? (int)g : 0x7fffffff;
    float f32 = 0.0f, ph32 = 0.0f, step = 0.0f;
    if (active) {
        double f, phic;
        fit_decode(c, J, 0, f_min, df, 0.0, FIT_TWO_PI / (double)J, f_min, f_max, f, phic);
        fit_candidate(SH, f, phic, n, sr, f32, ph32);
        step = lfo_step(SH, f32, ph32, sr);
    }
    double St = 0.0, Stt = 0.0, Sty = 0.0;
    for (int base = 0; base < n; base += MX_TRACK_FIT_ROW_TILE) {
        const int len = min(MX_TRACK_FIT_ROW_TILE, n - base);
        __syncthreads();                                        // the tile before is read out
        for (int j = tid; j < len; j += TRACK_TILE_THREADS) tile[j] = yc[base + j];
        __syncthreads();
        if (active) {
            for (int j = 0; j < len; ++j) {
                const double t = (double)lfo_value(base + j, 0, step, ph32, SH, 1.0f);
                St += t;
                Stt = fma(t, t, Stt);
                Sty = fma(t, tile[j], Sty);
            }
        }
    }
    FitBest best;
    best.R = active ? fit_objective(St, Stt, Sty, Syy, n, nullptr) : INFINITY;
    best.c = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double R2 = __shfl_xor(best.R, o, MX_WAVE);
        const int c2 = __shfl_xor(best.c, o, MX_WAVE);
        if (fit_less(R2, c2, best.R, best.c)) {
            best.R = R2;
            best.c = c2;
        }
    }
    if ((tid & (MX_WAVE - 1)) == 0) red[tid / MX_WAVE] = best;
    __syncthreads();
    best = red[0];
    for (int w = 1; w < TRACK_TILE_WAVES; ++w)
        if (fit_less(red[w].R, red[w].c, best.R, best.c)) best = red[w];
    return best;
}

__global__ __launch_bounds__(TRACK_TILE_THREADS) void track_coarse_kernel(
    const double *__restrict__ stats, const double *__restrict__ yc_all, long long b0, int n, float sr, double f_min, double f_max,
    double df, int J, long long ncand, int mask, FitBest *__restrict__ part)
{
    __shared__ double tile[MX_TRACK_FIT_ROW_TILE];
    __shared__ FitBest red[TRACK_TILE_WAVES];
    const int sh = (int)blockIdx.y;
    const size_t b = (size_t)b0 + blockIdx.z;
    const double Syy = stats[2 * b + 1];
    if (!((mask >> sh) & 1) || Syy == 0.0) return;              // uniform over the workgroup
    const double *yc = yc_all + b * (size_t)n;
    FitBest r;
    switch (sh) {
    case LFO_COS: r = track_coarse_tile<LFO_COS>(yc, n, sr, Syy, f_min, f_max, df, J, ncand, tile, red); break;
    case LFO_RECT_COS: r = track_coarse_tile<LFO_RECT_COS>(yc, n, sr, Syy, f_min, f_max, df, J, ncand, tile, red); break;
    case LFO_INV_RECT_COS: r = track_coarse_tile<LFO_INV_RECT_COS>(yc, n, sr, Syy, f_min, f_max, df, J, ncand, tile, red); break;
    case LFO_TRI: r = track_coarse_tile<LFO_TRI>(yc, n, sr, Syy, f_min, f_max, df, J, ncand, tile, red); break;
    case LFO_SAW: r = track_coarse_tile<LFO_SAW>(yc, n, sr, Syy, f_min, f_max, df, J, ncand, tile, red); break;
    case LFO_RSAW: r = track_coarse_tile<LFO_RSAW>(yc, n, sr, Syy, f_min, f_max, df, J, ncand, tile, red); break;
    default: r = track_coarse_tile<LFO_SQR>(yc, n, sr, Syy, f_min, f_max, df, J, ncand, tile, red); break;
    }
    if (threadIdx.x == 0) part[(b * FIT_N_SHAPES + (size_t)sh) * gridDim.x + blockIdx.x] = r;
}

__global__ __launch_bounds__(FIT_THREADS) void track_refine_kernel(
    const double *__restrict__ stats, const double *__restrict__ yc_all, const FitBest *__restrict__ part, long long ntiles,
    long long b0, int n, float sr, double f_min, double f_max, double df, int J, int L, int mask, double *__restrict__ res)
{
    __shared__ FitBest red[FIT_WAVES];
    const int sh = (int)blockIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    const double Syy = stats[2 * b + 1];
    if (!((mask >> sh) & 1) || Syy == 0.0) return;              // uniform over the workgroup
    const int tid = (int)threadIdx.x;
    const double *yc = yc_all + b * (size_t)n;
    const FitBest *p = part + (b * FIT_N_SHAPES + (size_t)sh) * (size_t)ntiles;

    FitBest best;
    best.R = INFINITY;
    best.c = 0x7fffffff;
    for (long long t = tid; t < ntiles; t += FIT_THREADS) {
        const FitBest v = p[t];
        if (fit_less(v.R, v.c, best.R, best.c)) best = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double R2 = __shfl_xor(best.R, o, MX_WAVE);
        const int c2 = __shfl_xor(best.c, o, MX_WAVE);
        if (fit_less(R2, c2, best.R, best.c)) {
            best.R = R2;
            best.c = c2;
        }
    }
    if ((tid & (MX_WAVE - 1)) == 0) red[tid / MX_WAVE] = best;
    __syncthreads();
    best = red[0];
    for (int w = 1; w < FIT_WAVES; ++w)
        if (fit_less(red[w].R, red[w].c, best.R, best.c)) best = red[w];

    double R0 = INFINITY, f0 = f_min, phi0 = 0.0;
    if (best.R < R0) {
        R0 = best.R;
        fit_decode(best.c, J, 0, f_min, df, 0.0, FIT_TWO_PI / (double)J, f_min, f_max, f0, phi0);
    }
    switch (sh) {
    case LFO_COS: fit_refine_rounds<LFO_COS>(yc, n, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_RECT_COS: fit_refine_rounds<LFO_RECT_COS>(yc, n, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_INV_RECT_COS: fit_refine_rounds<LFO_INV_RECT_COS>(yc, n, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_TRI: fit_refine_rounds<LFO_TRI>(yc, n, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_SAW: fit_refine_rounds<LFO_SAW>(yc, n, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_RSAW: fit_refine_rounds<LFO_RSAW>(yc, n, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    default: fit_refine_rounds<LFO_SQR>(yc, n, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    }
    if (tid == 0) {
        double *o = res + (b * FIT_N_SHAPES + (size_t)sh) * 3;
        o[0] = R0;
        o[1] = f0;
        o[2] = phi0;
    }
}

__global__ __launch_bounds__(MX_WAVE) void track_final_kernel(
    const double *__restrict__ stats, const double *__restrict__ yc_all, const double *__restrict__ res, long long b0, int n, float sr,
    double f_min, int mask, int *__restrict__ shape, float *__restrict__ rate_hz, float *__restrict__ phase, float *__restrict__ amp,
    float *__restrict__ offset, float *__restrict__ resid, float *__restrict__ per_shape)
{
    const size_t b = (size_t)b0 + blockIdx.x;
    const int lane = (int)threadIdx.x;
    const double mean = stats[2 * b], Syy = stats[2 * b + 1];
    float *ps = per_shape ? per_shape + b * FIT_N_SHAPES : nullptr;
    if (Syy == 0.0) {                                           // a constant row (uniform over the wave)
        if (lane == 0) {
            shape[b] = __ffs(mask) - 1;
            rate_hz[b] = (float)f_min;
            phase[b] = 0.0f;
            amp[b] = 0.0f;
            offset[b] = (float)mean;
            resid[b] = 0.0f;
        }
        if (ps && lane < FIT_N_SHAPES) ps[lane] = ((mask >> lane) & 1) ? 0.0f : INFINITY;
        return;
    }
    double bestR = INFINITY, bestF = f_min, bestP = 0.0;
    int bestS = -1;
    for (int sh = 0; sh < FIT_N_SHAPES; ++sh) {
        if (!((mask >> sh) & 1)) {
            if (ps && lane == 0) ps[sh] = INFINITY;
            continue;
        }
        const double *r = res + (b * FIT_N_SHAPES + (size_t)sh) * 3;
        const double R = r[0];
        if (ps && lane == 0) ps[sh] = (float)(R / Syy);
        if (R < bestR) {
            bestR = R;
            bestF = r[1];
            bestP = r[2];
            bestS = sh;
        }
    }
    const double *yc = yc_all + b * (size_t)n;
    float f32, ph32;
    fit_candidate(bestS, bestF, bestP, n, sr, f32, ph32);
    float fe = f32, pe = ph32;
    const float step = lfo_step(bestS, fe, pe, sr);
    double St = 0.0, Stt = 0.0, Sty = 0.0;
    for (int i = lane; i < n; i += MX_WAVE) {
        const double t = (double)lfo_value(i, 0, step, pe, bestS, 1.0f);
        St += t;
        Stt = fma(t, t, Stt);
        Sty = fma(t, yc[i], Sty);
    }
    St = wave_sum_f64(St);
    Stt = wave_sum_f64(Stt);
    Sty = wave_sum_f64(Sty);
    if (lane != 0) return;
    double a;
    fit_objective(St, Stt, Sty, Syy, n, &a);
    shape[b] = bestS;
    rate_hz[b] = f32;
    phase[b] = ph32;
    amp[b] = (float)a;
    offset[b] = (float)(mean - a * (St / (double)n));
    resid[b] = (float)(bestR / Syy);
}

// C ABI (track_fit_abi.h) -------------------------------------------------------------------------
struct TrackGrid { double df; long long K, ntiles, ws_bytes; };

// mx_lfo_fit's checks after the pointers, in its order, with K23's limits; the grid and the workspace's size
static int track_fit_grid(int64_t y_stride, int64_t B, int64_t n, float sr, float f_min, float f_max, int32_t shape_mask,
                          int32_t rate_div, int32_t J, int32_t L, TrackGrid &g)
{
    if (!(f_min > 0.0f) || !(f_max >= f_min) || !(f_max < sr * 0.5f)) return MX_ERR_ARG;
    if (shape_mask <= 0 || shape_mask >= (1 << FIT_N_SHAPES) || L < 0) return MX_ERR_ARG;
    if (n < FIT_MIN_N || n > MX_TRACK_FIT_MAX_N || J < 4 || J > 128 || L > 8 || rate_div < 1 || rate_div > 16)
        return MX_ERR_UNSUPPORTED;
    if (y_stride < n) return MX_ERR_ARG;
    g.df = 1.0 / ((double)rate_div * ((double)n / (double)sr));
    const double k = floor(((double)f_max - (double)f_min) / g.df) + 1.0;
    if (k > (double)MX_TRACK_FIT_MAX_K || k * (double)J >= 2147483648.0) return MX_ERR_UNSUPPORTED;
    g.K = (long long)k;
    g.ntiles = (g.K * J + MX_TRACK_FIT_CAND_TILE - 1) / MX_TRACK_FIT_CAND_TILE;
    // FitBest partials first (16-byte items), then yc, (mean, Syy) and (R, f, phic) per shape as doubles
    const double bytes = (double)B * ((double)FIT_N_SHAPES * (double)g.ntiles * 16.0 + 8.0 * ((double)n + 2.0 + 3.0 * FIT_N_SHAPES));
    if (bytes >= 4611686018427387904.0) return MX_ERR_UNSUPPORTED;
    g.ws_bytes = B * (FIT_N_SHAPES * g.ntiles * 16 + 8 * (n + 2 + 3 * FIT_N_SHAPES));
    return MX_OK;
}

MX_EXPORT int mx_track_fit_plan(int64_t B, int64_t n, float sr, float f_min, float f_max, int32_t shape_mask, int32_t rate_div,
                                int32_t J, int32_t L, int64_t *K, int64_t *ws_bytes)
{
    if (!K || !ws_bytes || B <= 0) return MX_ERR_ARG;
    TrackGrid g;
    const int rc = track_fit_grid(n, B, n, sr, f_min, f_max, shape_mask, rate_div, J, L, g);
    if (rc != MX_OK) return rc;
    *K = g.K;
    *ws_bytes = g.ws_bytes;
    return MX_OK;
}

MX_EXPORT int mx_track_fit(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, float f_min, float f_max,
                           int32_t shape_mask, int32_t rate_div, int32_t J, int32_t L, int32_t *shape, float *rate_hz, float *phase,
                           float *amp, float *offset, float *resid, float *per_shape_resid, void *ws, int64_t ws_bytes, void *stream)
{
    static_assert(sizeof(FitBest) == 16, "the workspace holds FitBest as 16-byte items");
    if (!y || !shape || !rate_hz || !phase || !amp || !offset || !resid || !ws || B <= 0) return MX_ERR_ARG;
    TrackGrid g;
    const int rc = track_fit_grid(y_stride, B, n, sr, f_min, f_max, shape_mask, rate_div, J, L, g);
    if (rc != MX_OK) return rc;
    if (((uintptr_t)ws & 15) != 0 || ws_bytes < g.ws_bytes) return MX_ERR_ARG;
    FitBest *part = (FitBest *)ws;
    double *yc = (double *)(part + (size_t)B * FIT_N_SHAPES * (size_t)g.ntiles);
    double *stats = yc + (size_t)B * (size_t)n;
    double *res = stats + 2 * (size_t)B;
    hipStream_t st = (hipStream_t)stream;
    for (int64_t b0 = 0; b0 < B; b0 += TRACK_MAX_ROWS) {
        const unsigned rows = (unsigned)(B - b0 < TRACK_MAX_ROWS ? B - b0 : TRACK_MAX_ROWS);
        hipLaunchKernelGGL(track_prep_kernel, dim3(rows), dim3(FIT_THREADS), 0, st, y, (long long)y_stride, (long long)b0, (int)n,
                           stats, yc);
        hipLaunchKernelGGL(track_coarse_kernel, dim3((unsigned)g.ntiles, FIT_N_SHAPES, rows), dim3(TRACK_TILE_THREADS), 0, st,
                           stats, yc, (long long)b0, (int)n, sr, (double)f_min, (double)f_max, g.df, (int)J, g.K * J, (int)shape_mask,
                           part);
        hipLaunchKernelGGL(track_refine_kernel, dim3(FIT_N_SHAPES, rows), dim3(FIT_THREADS), 0, st, stats, yc, part, g.ntiles,
                           (long long)b0, (int)n, sr, (double)f_min, (double)f_max, g.df, (int)J, (int)L, (int)shape_mask, res);
        hipLaunchKernelGGL(track_final_kernel, dim3(rows), dim3(MX_WAVE), 0, st, stats, yc, res, (long long)b0, (int)n, sr,
                           (double)f_min, (int)shape_mask, shape, rate_hz, phase, amp, offset, resid, per_shape_resid);
    }
    return mx_launch_status();
}
