// rate_track.hip -- K25: the rate contour of an LFO track whose rate moves (rate_track_abi.h has the definition) -- no
// counterpart in the reference.  The track is cut into S slices of W points; every slice gets K18's coarse grid of candidates
// (the node costs), a Viterbi path per (row, shape) joins one candidate a slice by rate and phase continuity, and K18's
// refinement polishes every slice from the path's candidate.
//
// Workspace (rate_track_plan has the size): per (row, slice) (mean, Syy); per (row, shape) the path's end (cost, state); per
// (row, shape, slice, state) one int32 back-pointer.  Launches:
// rate_stats_kernel   one 1024-thread workgroup per (slice, row): mean and Syy in K18's order (lanes by butterfly, then the 16
//     waves in order), so a slice has the statistics mx_lfo_fit gives the same points.
// rate_nodes_kernel   grid (candidate tile x shape, slice, row), 256 threads, one candidate a lane (the shape is uniform over
//     the workgroup, each its own instantiation, so lfo_value folds to one branch).  The centred slice is built in LDS once
//     (8 W bytes, dynamic: 5.4 KB at W = 690, so the wave slots and not LDS bound the occupancy); every lane reads the same
//     yc[i], a broadcast; the three fp64 accumulators run in ascending i with fma, as K18's do at nsub == 1.  Compute-bound: W
//     template evaluations (a cosf or an fmodf each) a lane, 16 bytes written per candidate.
// rate_path_kernel    one 1024-thread workgroup per (shape, row).  The column V_{s-1} sits in LDS (K J <= 8192 doubles, 64 KB);
//     lane t owns the targets t, t + 1024, ... (at most 8, kept in registers until the column is read out), scans the sources
//     (k_a, j_a), k_a = k_b - D .. k_b + D inside the grid, j_a ascending -- ascending a -- and keeps a source only when
//     strictly smaller.  The transition is formed with __dmul_rn / __dadd_rn / __ddiv_rn in the header's order; the 2 J - 1
//     quotients ((j_b - j_a) q) / J are divided once per workgroup into LDS (the same division, the same bits).
// rate_pick_kernel    one lane per row: the argmin over the allowed shapes, the backtrack, the path and the costs.
// rate_refine_kernel  one 1024-thread workgroup per (slice, row): the centred slice in LDS (32 KB), R0 at the path's candidate
//     by lane 0 in ascending i (the node's order), rounds 1..L through fit_refine_rounds, then amp / offset / resid as K18's
//     wave 0 writes them.
// No atomics; fixed orders throughout.
#include "lfo_fit_common.h"
#include "rate_track_abi.h"

#define RATE_TILE_THREADS MX_RATE_TRACK_CAND_TILE
#define RATE_PER_LANE (MX_RATE_TRACK_MAX_STATES / FIT_THREADS)

// starts[s], kept inside the row whatever the caller wrote
__device__ __forceinline__ long long rate_start(const long long *__restrict__ starts, int s, int n, int W)
{
    const long long v = starts[s];
    return v < 0 ? 0 : (v > (long long)(n - W) ? (long long)(n - W) : v);
}

__global__ __launch_bounds__(FIT_THREADS) void rate_stats_kernel(const float *__restrict__ y, long long y_stride,
                                                                 const long long *__restrict__ starts, int S, int n, int W,
                                                                 double *__restrict__ stats)
{
    __shared__ double redd[FIT_WAVES];
    const int s = (int)blockIdx.x;
    const size_t b = blockIdx.y;
    const int tid = (int)threadIdx.x, lane = tid & (MX_WAVE - 1), wave = tid / MX_WAVE;
    const float *row = y + b * (size_t)y_stride + rate_start(starts, s, n, W);

    double a = 0.0;
    for (int i = tid; i < W; i += FIT_THREADS) a += (double)row[i];
    a = wave_sum_f64(a);
    if (lane == 0) redd[wave] = a;
    __syncthreads();
    a = 0.0;
    for (int w = 0; w < FIT_WAVES; ++w) a += redd[w];
    const double mean = a / (double)W;
    double q = 0.0;
    for (int i = tid; i < W; i += FIT_THREADS) {
        const double v = (double)row[i] - mean;
        q = fma(v, v, q);
    }
    q = wave_sum_f64(q);
    __syncthreads();                                            // redd was read above
    if (lane == 0) redd[wave] = q;
    __syncthreads();
    if (tid != 0) return;
    double Syy = 0.0;
    for (int w = 0; w < FIT_WAVES; ++w) Syy += redd[w];
    double *o = stats + 2 * (b * (size_t)S + (size_t)s);
    o[0] = mean;
    o[1] = Syy;
}

// R of coarse candidate c of shape SH on the centred slice yc (LDS), the sums in ascending i
template <int SH>
__device__ __forceinline__ double rate_candidate_R(const double *yc, int W, float sr, double Syy, double f_min, double f_max,
                                                   double df, int J, int c)
{
    double f, phic;
    fit_decode(c, J, 0, f_min, df, 0.0, FIT_TWO_PI / (double)J, f_min, f_max, f, phic);
    float f32, ph32;
    fit_candidate(SH, f, phic, W, sr, f32, ph32);
    const float step = lfo_step(SH, f32, ph32, sr);
    double St = 0.0, Stt = 0.0, Sty = 0.0;
    for (int i = 0; i < W; ++i) {
        const double t = (double)lfo_value(i, 0, step, ph32, SH, 1.0f);
        St += t;
        Stt = fma(t, t, Stt);
        Sty = fma(t, yc[i], Sty);
    }
    return fit_objective(St, Stt, Sty, Syy, W, nullptr);
}

__device__ __forceinline__ double rate_candidate_R_of(int sh, const double *yc, int W, float sr, double Syy, double f_min,
                                                      double f_max, double df, int J, int c)
{
    switch (sh) {
    case LFO_COS: return rate_candidate_R<LFO_COS>(yc, W, sr, Syy, f_min, f_max, df, J, c);
    case LFO_RECT_COS: return rate_candidate_R<LFO_RECT_COS>(yc, W, sr, Syy, f_min, f_max, df, J, c);
    case LFO_INV_RECT_COS: return rate_candidate_R<LFO_INV_RECT_COS>(yc, W, sr, Syy, f_min, f_max, df, J, c);
    case LFO_TRI: return rate_candidate_R<LFO_TRI>(yc, W, sr, Syy, f_min, f_max, df, J, c);
    case LFO_SAW: return rate_candidate_R<LFO_SAW>(yc, W, sr, Syy, f_min, f_max, df, J, c);
    case LFO_RSAW: return rate_candidate_R<LFO_RSAW>(yc, W, sr, Syy, f_min, f_max, df, J, c);
    default: return rate_candidate_R<LFO_SQR>(yc, W, sr, Syy, f_min, f_max, df, J, c);
    }
}

__global__ __launch_bounds__(RATE_TILE_THREADS) void rate_nodes_kernel(
    const float *__restrict__ y, long long y_stride, const long long *__restrict__ starts, int S, int n, int W, float sr,
    double f_min, double f_max, double df, int J, int ncand, int ntiles, int mask, const double *__restrict__ stats,
    double *__restrict__ node)
{
    extern __shared__ double yc[];                              // W doubles
    const int sh = (int)blockIdx.x / ntiles, tile = (int)blockIdx.x - sh * ntiles;
    if (!((mask >> sh) & 1)) return;                            // uniform over the workgroup
    const int s = (int)blockIdx.y;
    const size_t b = blockIdx.z;
    const int tid = (int)threadIdx.x;
    const double *st = stats + 2 * (b * (size_t)S + (size_t)s);
    const double mean = st[0], Syy = st[1];
    const int c = tile * RATE_TILE_THREADS + tid;
    double *out = node + ((b * FIT_N_SHAPES + (size_t)sh) * (size_t)S + (size_t)s) * (size_t)ncand;
    if (Syy == 0.0) {                                           // a constant slice (uniform): every candidate costs 0
        if (c < ncand) out[c] = 0.0;
        return;
    }
    const float *row = y + b * (size_t)y_stride + rate_start(starts, s, n, W);
    for (int i = tid; i < W; i += RATE_TILE_THREADS) yc[i] = (double)row[i] - mean;
    __syncthreads();
    if (c >= ncand) return;
    out[c] = rate_candidate_R_of(sh, yc, W, sr, Syy, f_min, f_max, df, J, c) / Syy;
}

// the rate of grid bin k, as fit_decode forms it
__device__ __forceinline__ double rate_of_bin(int k, double f_min, double f_max, double df)
{
    const double f = __dadd_rn(f_min, __dmul_rn((double)k, df));
    return f < f_min ? f_min : (f > f_max ? f_max : f);
}

__global__ __launch_bounds__(FIT_THREADS) void rate_path_kernel(
    const long long *__restrict__ starts, int S, int n, int W, float sr, double f_min, double f_max, double df, int K, int J,
    int D, double rate_weight, double phase_weight, int mask, const double *__restrict__ node, int *__restrict__ back,
    double *__restrict__ end_cost, long long *__restrict__ end_state)
{
    __shared__ double V[MX_RATE_TRACK_MAX_STATES];
    __shared__ double turn[2 * 128 - 1];                        // ((j_b - j_a) q) / J at j_b - j_a + J - 1: one division each
    __shared__ FitBest red[FIT_WAVES];
    const int sh = (int)blockIdx.x;
    if (!((mask >> sh) & 1)) return;                            // uniform over the workgroup
    const size_t b = blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int ncand = K * J;
    const int q = (sh == LFO_RECT_COS || sh == LFO_INV_RECT_COS) ? 2 : 1;
    const size_t plane = (b * FIT_N_SHAPES + (size_t)sh) * (size_t)S;
    const double *nd = node + plane * (size_t)ncand;
    int *bp = back + plane * (size_t)ncand;

    for (int c = tid; c < ncand; c += FIT_THREADS) V[c] = nd[c];
    for (int d = tid; d < 2 * J - 1; d += FIT_THREADS) turn[d] = __ddiv_rn((double)((d - (J - 1)) * q), (double)J);
    __syncthreads();
    for (int s = 1; s < S; ++s) {
        const double dstart = (double)(rate_start(starts, s, n, W) - rate_start(starts, s - 1, n, W));
        const double *nds = nd + (size_t)s * (size_t)ncand;
        int *bps = bp + (size_t)s * (size_t)ncand;
        double vnew[RATE_PER_LANE];
        int anew[RATE_PER_LANE];
#pragma unroll
        for (int r = 0; r < RATE_PER_LANE; ++r) {
            const int c = tid + r * FIT_THREADS;
            vnew[r] = 0.0;
            anew[r] = 0;
            if (c >= ncand) continue;
            const int kb = c / J, jb = c - kb * J;
            const double fb = rate_of_bin(kb, f_min, f_max, df);
            const int k_lo = max(0, kb - D), k_hi = min(K - 1, kb + D);
            double best = INFINITY;
            int best_a = 0;
            for (int ka = k_lo; ka <= k_hi; ++ka) {
                const double fa = rate_of_bin(ka, f_min, f_max, df);
                const double adv = __ddiv_rn(__dmul_rn(__dmul_rn(0.5, __dadd_rn(fa, fb)), dstart), (double)sr);
                const int dk = kb - ka;
                const double tk = __dmul_rn(rate_weight, (double)(dk * dk));
                const double *Vk = V + ka * J;
                const double *tq = turn + jb + (J - 1);
                for (int ja = 0; ja < J; ++ja) {
                    double m = __dadd_rn(tq[-ja], -adv);
                    m = __dadd_rn(m, -rint(m));
                    const double tr = __dadd_rn(tk, __dmul_rn(phase_weight, __dmul_rn(m, m)));
                    const double v = __dadd_rn(Vk[ja], tr);
                    if (v < best) {                             // ascending a: ties stay with the lowest
                        best = v;
                        best_a = ka * J + ja;
                    }
                }
            }
            vnew[r] = __dadd_rn(nds[c], best);
            anew[r] = best_a;
        }
        __syncthreads();                                        // the column before is read out
#pragma unroll
        for (int r = 0; r < RATE_PER_LANE; ++r) {
            const int c = tid + r * FIT_THREADS;
            if (c < ncand) {
                V[c] = vnew[r];
                bps[c] = anew[r];
            }
        }
        __syncthreads();
    }
    // the end: the argmin of the last column under fit_less (value, then the lowest state)
    FitBest best;
    best.R = INFINITY;
    best.c = 0x7fffffff;
    for (int c = tid; c < ncand; c += FIT_THREADS)
        if (fit_less(V[c], c, best.R, best.c)) {
            best.R = V[c];
            best.c = c;
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
    if (tid != 0) return;
    best = red[0];
    for (int w = 1; w < FIT_WAVES; ++w)
        if (fit_less(red[w].R, red[w].c, best.R, best.c)) best = red[w];
    end_cost[b * FIT_N_SHAPES + (size_t)sh] = best.R;
    end_state[b * FIT_N_SHAPES + (size_t)sh] = best.c;
}

__global__ __launch_bounds__(MX_WAVE) void rate_pick_kernel(int B, int S, int ncand, int J, int mask, const int *__restrict__ back,
                                                            const double *__restrict__ end_cost,
                                                            const long long *__restrict__ end_state, int *__restrict__ shape,
                                                            int *__restrict__ grid_k, int *__restrict__ grid_j,
                                                            float *__restrict__ cost, float *__restrict__ per_shape)
{
    const int b = (int)(blockIdx.x * MX_WAVE + threadIdx.x);
    if (b >= B) return;
    double bestV = INFINITY;
    int bestS = -1;
    for (int sh = 0; sh < FIT_N_SHAPES; ++sh) {
        if (!((mask >> sh) & 1)) {
            per_shape[(size_t)b * FIT_N_SHAPES + sh] = INFINITY;
            continue;
        }
        const double v = end_cost[(size_t)b * FIT_N_SHAPES + sh];
        per_shape[(size_t)b * FIT_N_SHAPES + sh] = (float)v;
        if (bestS < 0 || v < bestV) {                           // ties to the lowest id
            bestV = v;
            bestS = sh;
        }
    }
    shape[b] = bestS;
    cost[b] = (float)bestV;
    const int *bp = back + ((size_t)b * FIT_N_SHAPES + (size_t)bestS) * (size_t)S * (size_t)ncand;
    int c = (int)end_state[(size_t)b * FIT_N_SHAPES + bestS];
    if (c < 0 || c >= ncand) c = 0;                             // a column of NaN has no argmin: stay inside the tables
    for (int s = S - 1; s >= 0; --s) {
        const int k = c / J;
        grid_k[(size_t)b * S + s] = k;
        grid_j[(size_t)b * S + s] = c - k * J;
        if (s > 0) c = bp[(size_t)s * (size_t)ncand + c];
    }
}

__global__ __launch_bounds__(FIT_THREADS) void rate_refine_kernel(
    const float *__restrict__ y, long long y_stride, const long long *__restrict__ starts, int S, int n, int W, float sr,
    double f_min, double f_max, double df, int K, int J, int L, const double *__restrict__ stats, const int *__restrict__ shape,
    const int *__restrict__ grid_k, const int *__restrict__ grid_j, float *__restrict__ rate_hz, float *__restrict__ phase,
    float *__restrict__ amp, float *__restrict__ offset, float *__restrict__ resid)
{
    __shared__ double yc[MX_RATE_TRACK_MAX_W];
    __shared__ FitBest red[FIT_WAVES];
    __shared__ double r_path;
    const int s = (int)blockIdx.x;
    const size_t b = blockIdx.y;
    const size_t o = b * (size_t)S + (size_t)s;
    const int tid = (int)threadIdx.x, lane = tid & (MX_WAVE - 1), wave = tid / MX_WAVE;
    const double mean = stats[2 * o], Syy = stats[2 * o + 1];
    int sh = shape[b], k = grid_k[o], j = grid_j[o];
    sh = sh < 0 ? 0 : (sh >= FIT_N_SHAPES ? FIT_N_SHAPES - 1 : sh);     // inputs of this launch: kept inside the grid
    k = k < 0 ? 0 : (k >= K ? K - 1 : k);
    j = j < 0 ? 0 : (j >= J ? J - 1 : j);
    double f0, phi0;
    fit_decode(k * J + j, J, 0, f_min, df, 0.0, FIT_TWO_PI / (double)J, f_min, f_max, f0, phi0);
    if (Syy == 0.0) {                                           // a constant slice (uniform): the path's grid candidate
        if (tid == 0) {
            float f32, ph32;
            fit_candidate(sh, f0, phi0, W, sr, f32, ph32);
            rate_hz[o] = f32;
            phase[o] = ph32;
            amp[o] = 0.0f;
            offset[o] = (float)mean;
            resid[o] = 0.0f;
        }
        return;
    }
    const float *row = y + b * (size_t)y_stride + rate_start(starts, s, n, W);
    for (int i = tid; i < W; i += FIT_THREADS) yc[i] = (double)row[i] - mean;
    __syncthreads();
    if (tid == 0) r_path = rate_candidate_R_of(sh, yc, W, sr, Syy, f_min, f_max, df, J, k * J + j);
    __syncthreads();
    double R0 = r_path;
    switch (sh) {
    case LFO_COS: fit_refine_rounds<LFO_COS>(yc, W, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_RECT_COS: fit_refine_rounds<LFO_RECT_COS>(yc, W, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_INV_RECT_COS: fit_refine_rounds<LFO_INV_RECT_COS>(yc, W, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_TRI: fit_refine_rounds<LFO_TRI>(yc, W, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_SAW: fit_refine_rounds<LFO_SAW>(yc, W, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    case LFO_RSAW: fit_refine_rounds<LFO_RSAW>(yc, W, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    default: fit_refine_rounds<LFO_SQR>(yc, W, sr, Syy, f_min, f_max, df, J, L, red, R0, f0, phi0); break;
    }

    // amp and offset at the winner: wave 0, the lanes striding along the slice, as in lfo_fit_kernel
    if (wave != 0) return;
    float f32, ph32;
    fit_candidate(sh, f0, phi0, W, sr, f32, ph32);
    float fe = f32, pe = ph32;
    const float step = lfo_step(sh, fe, pe, sr);
    double St = 0.0, Stt = 0.0, Sty = 0.0;
    for (int i = lane; i < W; i += MX_WAVE) {
        const double t = (double)lfo_value(i, 0, step, pe, sh, 1.0f);
        St += t;
        Stt = fma(t, t, Stt);
        Sty = fma(t, yc[i], Sty);
    }
    St = wave_sum_f64(St);
    Stt = wave_sum_f64(Stt);
    Sty = wave_sum_f64(Sty);
    if (lane != 0) return;
    double a;
    fit_objective(St, Stt, Sty, Syy, W, &a);
    rate_hz[o] = f32;
    phase[o] = ph32;
    amp[o] = (float)a;
    offset[o] = (float)(mean - a * (St / (double)W));
    resid[o] = (float)(R0 / Syy);
}

// C ABI (rate_track_abi.h) ------------------------------------------------------------------------
struct RateGrid { double df; long long K, ncand, ntiles, node_bytes, ws_bytes; };

// the plan's checks, in the header's order; the grid and the buffers' sizes
static int rate_track_grid(int64_t y_stride, int64_t B, int64_t n, float sr, int64_t S, int64_t W, float f_min, float f_max,
                           int32_t shape_mask, int32_t rate_div, int32_t J, int32_t L, int32_t D, RateGrid &g)
{
    if (B <= 0) return MX_ERR_ARG;
    if (!(f_min > 0.0f) || !(f_max >= f_min) || !(f_max < sr * 0.5f)) return MX_ERR_ARG;
    if (shape_mask <= 0 || shape_mask >= (1 << FIT_N_SHAPES) || L < 0) return MX_ERR_ARG;
    if (W < MX_RATE_TRACK_MIN_W || W > MX_RATE_TRACK_MAX_W || J < 4 || J > 128 || L > 8 || rate_div < 1 || rate_div > 16 ||
        n > MX_RATE_TRACK_MAX_N || B > MX_RATE_TRACK_MAX_ROWS || S < 1 || S > MX_RATE_TRACK_MAX_S || D < 0 || D > MX_RATE_TRACK_MAX_D)
        return MX_ERR_UNSUPPORTED;
    if (n < W || y_stride < n) return MX_ERR_ARG;
    g.df = 1.0 / ((double)rate_div * ((double)W / (double)sr));
    const double k = floor(((double)f_max - (double)f_min) / g.df) + 1.0;
    if (k * (double)J > (double)MX_RATE_TRACK_MAX_STATES) return MX_ERR_UNSUPPORTED;
    g.K = (long long)k;
    g.ncand = g.K * J;
    g.ntiles = (g.ncand + MX_RATE_TRACK_CAND_TILE - 1) / MX_RATE_TRACK_CAND_TILE;
    const long long cells = B * FIT_N_SHAPES * S * g.ncand;     // <= 65535 * 7 * 16384 * 8192 < 2^63 / 8
    g.node_bytes = 8 * cells;
    // (mean, Syy) per (row, slice), then the ends' costs and states per (row, shape), then the back-pointers
    g.ws_bytes = (8 * (2 * B * S + 2 * B * FIT_N_SHAPES) + 4 * cells + 15) / 16 * 16;
    return MX_OK;
}

struct RateWs { double *stats, *end_cost; long long *end_state; int *back; };

static RateWs rate_ws(void *ws, int64_t B, int64_t S)
{
    RateWs w;
    w.stats = (double *)ws;
    w.end_cost = w.stats + 2 * (size_t)B * (size_t)S;
    w.end_state = (long long *)(w.end_cost + (size_t)B * FIT_N_SHAPES);
    w.back = (int *)(w.end_state + (size_t)B * FIT_N_SHAPES);
    return w;
}

MX_EXPORT int mx_rate_track_plan(int64_t B, int64_t n, float sr, int64_t S, int64_t W, float f_min, float f_max,
                                 int32_t shape_mask, int32_t rate_div, int32_t J, int32_t L, int32_t D, int64_t *K,
                                 int64_t *node_bytes, int64_t *ws_bytes)
{
    if (!K || !node_bytes || !ws_bytes) return MX_ERR_ARG;
    RateGrid g;
    const int rc = rate_track_grid(n, B, n, sr, S, W, f_min, f_max, shape_mask, rate_div, J, L, D, g);
    if (rc != MX_OK) return rc;
    *K = g.K;
    *node_bytes = g.node_bytes;
    *ws_bytes = g.ws_bytes;
    return MX_OK;
}

static bool rate_buffers_ok(const void *node, int64_t node_bytes, const void *ws, int64_t ws_bytes, const RateGrid &g)
{
    return ((uintptr_t)node & 15) == 0 && ((uintptr_t)ws & 15) == 0 && node_bytes >= g.node_bytes && ws_bytes >= g.ws_bytes;
}

MX_EXPORT int mx_rate_track_nodes(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, const int64_t *starts,
                                  int64_t S, int64_t W, float f_min, float f_max, int32_t shape_mask, int32_t rate_div, int32_t J,
                                  double *node, int64_t node_bytes, void *ws, int64_t ws_bytes, void *stream)
{
    if (!y || !starts || !node || !ws) return MX_ERR_ARG;
    RateGrid g;
    const int rc = rate_track_grid(y_stride, B, n, sr, S, W, f_min, f_max, shape_mask, rate_div, J, 0, 0, g);
    if (rc != MX_OK) return rc;
    if (!rate_buffers_ok(node, node_bytes, ws, ws_bytes, g)) return MX_ERR_ARG;
    const RateWs w = rate_ws(ws, B, S);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rate_stats_kernel, dim3((unsigned)S, (unsigned)B), dim3(FIT_THREADS), 0, st, y, (long long)y_stride,
                       (const long long *)starts, (int)S, (int)n, (int)W, w.stats);
    hipLaunchKernelGGL(rate_nodes_kernel, dim3((unsigned)(g.ntiles * FIT_N_SHAPES), (unsigned)S, (unsigned)B),
                       dim3(RATE_TILE_THREADS), (size_t)W * sizeof(double), st, y, (long long)y_stride, (const long long *)starts,
                       (int)S, (int)n, (int)W, sr, (double)f_min, (double)f_max, g.df, (int)J, (int)g.ncand, (int)g.ntiles,
                       (int)shape_mask, w.stats, node);
    return mx_launch_status();
}

MX_EXPORT int mx_rate_track_path(int64_t B, int64_t n, float sr, const int64_t *starts, int64_t S, int64_t W, float f_min,
                                 float f_max, int32_t shape_mask, int32_t rate_div, int32_t J, int32_t D, double rate_weight,
                                 double phase_weight, const double *node, int64_t node_bytes, void *ws, int64_t ws_bytes,
                                 int32_t *shape, int32_t *grid_k, int32_t *grid_j, float *cost, float *per_shape_cost, void *stream)
{
    static_assert(sizeof(FitBest) == 16 && RATE_PER_LANE * FIT_THREADS == MX_RATE_TRACK_MAX_STATES, "the path's LDS plan");
    if (!starts || !node || !ws || !shape || !grid_k || !grid_j || !cost || !per_shape_cost) return MX_ERR_ARG;
    RateGrid g;
    const int rc = rate_track_grid(n, B, n, sr, S, W, f_min, f_max, shape_mask, rate_div, J, 0, D, g);
    if (rc != MX_OK) return rc;
    if (!(rate_weight >= 0.0) || !(phase_weight >= 0.0) || !(rate_weight < INFINITY) || !(phase_weight < INFINITY))
        return MX_ERR_ARG;
    if (!rate_buffers_ok(node, node_bytes, ws, ws_bytes, g)) return MX_ERR_ARG;
    const RateWs w = rate_ws(ws, B, S);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rate_path_kernel, dim3(FIT_N_SHAPES, (unsigned)B), dim3(FIT_THREADS), 0, st, (const long long *)starts,
                       (int)S, (int)n, (int)W, sr, (double)f_min, (double)f_max, g.df, (int)g.K, (int)J, (int)D, rate_weight,
                       phase_weight, (int)shape_mask, node, w.back, w.end_cost, w.end_state);
    hipLaunchKernelGGL(rate_pick_kernel, dim3((unsigned)((B + MX_WAVE - 1) / MX_WAVE)), dim3(MX_WAVE), 0, st, (int)B, (int)S,
                       (int)g.ncand, (int)J, (int)shape_mask, w.back, w.end_cost, w.end_state, shape, grid_k, grid_j, cost,
                       per_shape_cost);
    return mx_launch_status();
}

MX_EXPORT int mx_rate_track_refine(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, const int64_t *starts,
                                   int64_t S, int64_t W, float f_min, float f_max, int32_t shape_mask, int32_t rate_div, int32_t J,
                                   int32_t L, const int32_t *shape, const int32_t *grid_k, const int32_t *grid_j, float *rate_hz,
                                   float *phase, float *amp, float *offset, float *resid, void *ws, int64_t ws_bytes, void *stream)
{
    if (!y || !starts || !shape || !grid_k || !grid_j || !rate_hz || !phase || !amp || !offset || !resid || !ws) return MX_ERR_ARG;
    RateGrid g;
    const int rc = rate_track_grid(y_stride, B, n, sr, S, W, f_min, f_max, shape_mask, rate_div, J, L, 0, g);
    if (rc != MX_OK) return rc;
    if (((uintptr_t)ws & 15) != 0 || ws_bytes < g.ws_bytes) return MX_ERR_ARG;
    const RateWs w = rate_ws(ws, B, S);
    hipLaunchKernelGGL(rate_refine_kernel, dim3((unsigned)S, (unsigned)B), dim3(FIT_THREADS), 0, (hipStream_t)stream, y,
                       (long long)y_stride, (const long long *)starts, (int)S, (int)n, (int)W, sr, (double)f_min, (double)f_max,
                       g.df, (int)g.K, (int)J, (int)L, w.stats, shape, grid_k, grid_j, rate_hz, phase, amp, offset, resid);
    return mx_launch_status();
}
