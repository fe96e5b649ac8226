// lfo_fit.hip -- K18: the inverse of K1 (mx_lfo_synth): rate, phase and shape of an LFO row, by a grid search with refinement
// over the templates lfo_value (lfo_common.h) produces -- no counterpart in the reference.
//
// A candidate is (shape s, rate f, centre phase phic).  Its template is t_i = lfo_value(i, 0, step, ph, s, 1), with f rounded
// to fp32 once, step = lfo_step(...) (the rectified cosines halve f and ph as in synthesis) and ph chosen so that the
// template's own argument at the middle of the row, position (n + 1) / 2, is phic:
//     ph_eff = (phic - step_eff (n + 1) / 2) mod 2 pi;   ph = ph_eff, or 2 (ph_eff mod pi) for the two rectified shapes,
// formed in fp64 and rounded to fp32 once (a value that rounds up to fl32(2 pi) > 2 pi becomes 0: ph is a legal phase of
// make_mod_signal).  So offset + amp * mx_lfo_synth(rate_hz, phase, shape) re-creates the best template bit for bit.
// Objective, fp64, with yc = y - mean(y):  Syy = sum yc^2,  St = sum t,  Stt = sum t^2 - St^2 / n,  Sty = sum t yc,
//     a = Sty / Stt if Stt > 0 and Sty > 0 else 0;   R = Syy - a Sty;   b = mean(y) - a St / n.
// a >= 0 on purpose: with a free sign saw / rsaw and rect_cos / inv_rect_cos are one family and the shape is not identifiable.
// Search per shape: coarse grid f_k = f_min + k df (k < K), phi_j = j (2 pi / J), argmin R, ties to the lowest (k, j); then L
// rounds of the 5 x 5 points f0 + i df / 2^l (clamped into the window), (phi0 + j (2 pi / J) / 2^l) mod 2 pi, i, j in -2..2,
// a point replacing the best only when strictly smaller, in (i, j) order; then the argmin over the allowed shapes, ties to the
// lowest id.
//
// lfo_fit_kernel  one 1024-thread workgroup per row; the shapes are taken one after the other (the shape is uniform over the
//     workgroup, each shape its own instantiation of the search, so lfo_value folds to one branch).  The centred row sits in
//     LDS as fp64 (32 KB at n = 4096).  A stage (the coarse grid, or one refinement round) hands every candidate to nsub
//     consecutive lanes (nsub a power of two <= 64: 1 on a grid of >= 1024 candidates, 32 in a 25-point round); lane sub
//     takes the points sub, sub + nsub, ... with three fp64 accumulators; the lanes of a candidate are combined by a butterfly
//     and the candidates by a (value, index) argmin: lanes, then the 16 waves through LDS.  With nsub == 1 every lane reads the
//     same yc[i] (a broadcast).  No atomics, no workspace, fixed order: the same arguments give the same bits.
//     amp and offset are re-evaluated at the winner by wave 0.
// Compute-bound: K J n template evaluations per shape and row (4.4 M per row at the default grid and n = 345), each a cosf or
// an fmodf; the row is read once.
// The candidate arithmetic, the objective, the argmin's order and fit_stage live in lfo_fit_common.h: track_fit.hip (K23), the
// same fit on a grid of workgroups for rows and grids beyond the limits below, shares them.
#include "lfo_fit_common.h"

#define FIT_MAX_N 4096
#define FIT_MAX_K 512

// coarse grid and L refinement rounds of shape SH: R0 and the (f0, phi0) it was found at
template <int SH>
__device__ void fit_shape(const double *yc, int n, float sr, double Syy, double f_min, double f_max, double df, int K, int J,
                          int L, FitBest *red, double &R0, double &f0, double &phi0)
{
    const double dphi = FIT_TWO_PI / (double)J;
    R0 = INFINITY;
    f0 = f_min;
    phi0 = 0.0;
    for (int l = 0; l <= L; ++l) {
        const double scale = 1.0 / (double)(1 << l);
        const int width = l == 0 ? J : 5, off = l == 0 ? 0 : 2, ncand = l == 0 ? K * J : 25;
        const double fbase = l == 0 ? f_min : f0, pbase = l == 0 ? 0.0 : phi0;
        const FitBest r = fit_stage<SH>(yc, n, sr, Syy, width, off, ncand, fbase, df * scale, pbase, dphi * scale, f_min, f_max,
                                        red);
        if (r.R < R0) {
            R0 = r.R;
            fit_decode(r.c, width, off, fbase, df * scale, pbase, dphi * scale, f_min, f_max, f0, phi0);
        }
    }
}

__global__ __launch_bounds__(FIT_THREADS) void lfo_fit_kernel(
    const float *__restrict__ y, long long y_stride, int n, float sr, double f_min, double f_max, double df, int K, int mask,
    int J, int L, int *__restrict__ shape, float *__restrict__ rate_hz, float *__restrict__ phase, float *__restrict__ amp,
    float *__restrict__ offset, float *__restrict__ resid, float *__restrict__ per_shape)
{
    __shared__ double yc[FIT_MAX_N];
    __shared__ FitBest red[FIT_WAVES];
    __shared__ double redd[FIT_WAVES];
    const size_t b = blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & (MX_WAVE - 1), wave = tid / MX_WAVE;
    const float *row = y + b * (size_t)y_stride;

    // mean and Syy: lanes by butterfly, then the waves in order
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
    __syncthreads();                                            // also: yc is complete
    double Syy = 0.0;
    for (int w = 0; w < FIT_WAVES; ++w) Syy += redd[w];

    float *ps = per_shape ? per_shape + b * FIT_N_SHAPES : nullptr;
    if (Syy == 0.0) {                                           // a constant row (uniform over the workgroup)
        if (tid == 0) {
            shape[b] = __ffs(mask) - 1;
            rate_hz[b] = (float)f_min;
            phase[b] = 0.0f;
            amp[b] = 0.0f;
            offset[b] = (float)mean;
            resid[b] = 0.0f;
        }
        if (ps && tid < FIT_N_SHAPES) ps[tid] = ((mask >> tid) & 1) ? 0.0f : INFINITY;
        return;
    }

    double bestR = INFINITY, bestF = f_min, bestP = 0.0;
    int bestS = -1;
    for (int sh = 0; sh < FIT_N_SHAPES; ++sh) {
        if (!((mask >> sh) & 1)) {
            if (ps && tid == 0) ps[sh] = INFINITY;
            continue;
        }
        double R, f, p;
        switch (sh) {
        case LFO_COS: fit_shape<LFO_COS>(yc, n, sr, Syy, f_min, f_max, df, K, J, L, red, R, f, p); break;
        case LFO_RECT_COS: fit_shape<LFO_RECT_COS>(yc, n, sr, Syy, f_min, f_max, df, K, J, L, red, R, f, p); break;
        case LFO_INV_RECT_COS: fit_shape<LFO_INV_RECT_COS>(yc, n, sr, Syy, f_min, f_max, df, K, J, L, red, R, f, p); break;
        case LFO_TRI: fit_shape<LFO_TRI>(yc, n, sr, Syy, f_min, f_max, df, K, J, L, red, R, f, p); break;
        case LFO_SAW: fit_shape<LFO_SAW>(yc, n, sr, Syy, f_min, f_max, df, K, J, L, red, R, f, p); break;
        case LFO_RSAW: fit_shape<LFO_RSAW>(yc, n, sr, Syy, f_min, f_max, df, K, J, L, red, R, f, p); break;
        default: fit_shape<LFO_SQR>(yc, n, sr, Syy, f_min, f_max, df, K, J, L, red, R, f, p); break;
        }
        if (ps && tid == 0) ps[sh] = (float)(R / Syy);
        if (R < bestR) {
            bestR = R;
            bestF = f;
            bestP = p;
            bestS = sh;
        }
    }

    // amp and offset at the winner: wave 0, the lanes striding along the row
    if (wave != 0) return;
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

// C ABI ---------------------------------------------------------------------------------------
// y: B rows of n fp32 points, y_stride floats apart; sr the rate of the points; [f_min, f_max] the rate window in Hz;
// shape_mask bit s allows shape id s of lfo_common.h; rate_div, J, L the grid (df = sr / (rate_div n), J centre phases, L
// refinement rounds).  Outputs (B,): shape int32, the rest fp32; per_shape_resid (B, 7) fp32 optional (+inf where not allowed).
MX_EXPORT int mx_lfo_fit(const float *y, int64_t y_stride, int64_t B, int64_t n, float sr, float f_min, float f_max,
                         int32_t shape_mask, int32_t rate_div, int32_t J, int32_t L, int32_t *shape, float *rate_hz,
                         float *phase, float *amp, float *offset, float *resid, float *per_shape_resid, void *stream)
{
    if (!y || !shape || !rate_hz || !phase || !amp || !offset || !resid || B <= 0) return MX_ERR_ARG;
    if (!(f_min > 0.0f) || !(f_max >= f_min) || !(f_max < sr * 0.5f)) return MX_ERR_ARG;
    if (shape_mask <= 0 || shape_mask >= (1 << FIT_N_SHAPES) || L < 0) return MX_ERR_ARG;
    if (n < FIT_MIN_N || n > FIT_MAX_N || J < 4 || J > 128 || L > 8 || rate_div < 1 || rate_div > 16 || B > 0x7fffffffll)
        return MX_ERR_UNSUPPORTED;
    if (y_stride < n) return MX_ERR_ARG;
    const double df = 1.0 / ((double)rate_div * ((double)n / (double)sr));
    const double k = floor(((double)f_max - (double)f_min) / df) + 1.0;
    if (k > (double)FIT_MAX_K) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lfo_fit_kernel, dim3((unsigned)B), dim3(FIT_THREADS), 0, (hipStream_t)stream, y, (long long)y_stride,
                       (int)n, sr, (double)f_min, (double)f_max, df, (int)k, (int)shape_mask, (int)J, (int)L, shape, rate_hz,
                       phase, amp, offset, resid, per_shape_resid);
    return mx_launch_status();
}
