// lfo_fit_common.h -- what the two LFO fits share (lfo_fit.hip, K18: one workgroup per row; track_fit.hip, K23: a grid of
// candidate tiles): the candidate's fp32 (rate, phase), the decoding of a candidate index, the objective, the order of the
// argmin, and one search stage of a 1024-thread workgroup over a centred fp64 row.  lfo_fit.hip has the definition of the fit.
// rate_track.hip (K25) evaluates the same candidates per slice of a track and runs the same refinement rounds, which K23 and
// K25 share as fit_refine_rounds.
#pragma once
#include "lfo_common.h"

#define FIT_THREADS 1024
#define FIT_WAVES (FIT_THREADS / MX_WAVE)
#define FIT_MIN_N 16
#define FIT_N_SHAPES 7
#define FIT_TWO_PI 6.283185307179586
#define FIT_PI 3.141592653589793

struct FitBest { double R; int c; };

// the fp32 (rate, phase) of a candidate: what mx_lfo_synth is given to synthesise its template
__device__ __forceinline__ void fit_candidate(int sh, double f, double phic, int n, float sr, float &f32, float &ph32)
{
    const float TWO_PI_F = 6.283185307179586f;
    f32 = (float)f;
    float fe = f32, unused = 0.0f;
    const float step = lfo_step(sh, fe, unused, sr);
    double p = fmod(phic - (double)step * (0.5 * (double)(n + 1)), FIT_TWO_PI);
    if (p < 0.0) p += FIT_TWO_PI;
    if (sh == LFO_RECT_COS || sh == LFO_INV_RECT_COS) p = 2.0 * fmod(p, FIT_PI);
    ph32 = (float)p;
    if (ph32 >= TWO_PI_F) ph32 = 0.0f;
}

// candidate c of a stage: (ki, ji) = (c / width - off, c % width - off) steps from (fbase, pbase)
__device__ __forceinline__ void fit_decode(int c, int width, int off, double fbase, double fstep, double pbase, double pstep,
                                           double f_min, double f_max, double &f, double &phic)
{
    const int ki = c / width, ji = c - ki * width;
    f = fbase + (double)(ki - off) * fstep;
    f = f < f_min ? f_min : (f > f_max ? f_max : f);
    phic = fmod(pbase + (double)(ji - off) * pstep, FIT_TWO_PI);
    if (phic < 0.0) phic += FIT_TWO_PI;
}

__device__ __forceinline__ double fit_objective(double St, double Stt, double Sty, double Syy, int n, double *a_out)
{
    const double var = Stt - St * (St / (double)n);
    const double a = (var > 0.0 && Sty > 0.0) ? Sty / var : 0.0;
    if (a_out) *a_out = a;
    return Syy - a * Sty;
}

__device__ __forceinline__ bool fit_less(double R2, int c2, double R, int c)
{
    return R2 < R || (R2 == R && c2 < c);
}

__device__ __forceinline__ int fit_nsub(int ncand)
{
    int nsub = 1;
    while (nsub < MX_WAVE && ncand * nsub * 2 <= FIT_THREADS) nsub *= 2;
    return nsub;
}

// one stage for shape SH: the (R, c) argmin over its ncand candidates, returned to every thread
template <int SH>
__device__ __forceinline__ FitBest fit_stage(const double *yc, int n, float sr, double Syy, int width, int off, int ncand,
                                             double fbase, double fstep, double pbase, double pstep, double f_min, double f_max,
                                             FitBest *red)
{
    const int tid = (int)threadIdx.x;
    const int nsub = fit_nsub(ncand);
    const int lsub = 31 - __clz(nsub);
    const int total = ncand * nsub;
    FitBest best;
    best.R = INFINITY;
    best.c = 0x7fffffff;
    for (int base = 0; base < total; base += FIT_THREADS) {     // uniform: every lane reaches the butterfly
        const int g = base + tid;
        const int c = g >> lsub, sub = g & (nsub - 1);
        double St = 0.0, Stt = 0.0, Sty = 0.0;
        if (c < ncand) {
            double f, phic;
            fit_decode(c, width, off, fbase, fstep, pbase, pstep, f_min, f_max, f, phic);
            float f32, ph32;
            fit_candidate(SH, f, phic, n, sr, f32, ph32);
            const float step = lfo_step(SH, f32, ph32, sr);
            for (int i = sub; i < n; i += nsub) {
                const double t = (double)lfo_value(i, 0, step, ph32, SH, 1.0f);
                St += t;
                Stt = fma(t, t, Stt);
                Sty = fma(t, yc[i], Sty);
            }
        }
        for (int o = nsub >> 1; o > 0; o >>= 1) {
            St += __shfl_xor(St, o, MX_WAVE);
            Stt += __shfl_xor(Stt, o, MX_WAVE);
            Sty += __shfl_xor(Sty, o, MX_WAVE);
        }
        if (c < ncand && sub == 0) {
            const double R = fit_objective(St, Stt, Sty, Syy, n, nullptr);
            if (R < best.R) {                                   // a thread's candidates come in ascending c
                best.R = R;
                best.c = c;
            }
        }
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
    __syncthreads();                                            // red may still be read from the stage before
    if ((tid & (MX_WAVE - 1)) == 0) red[tid / MX_WAVE] = best;
    __syncthreads();
    best = red[0];
    for (int w = 1; w < FIT_WAVES; ++w)
        if (fit_less(red[w].R, red[w].c, best.R, best.c)) best = red[w];
    return best;
}

// rounds 1..L of shape SH from the coarse (R0, f0, phi0), as fit_shape of lfo_fit.hip runs them
template <int SH>
__device__ void fit_refine_rounds(const double *yc, int n, float sr, double Syy, double f_min, double f_max, double df, int J, int L,
                                   FitBest *red, double &R0, double &f0, double &phi0)
{
    const double dphi = FIT_TWO_PI / (double)J;
    for (int l = 1; l <= L; ++l) {
        const double scale = 1.0 / (double)(1 << l);
        const double fbase = f0, pbase = phi0;
        const FitBest r = fit_stage<SH>(yc, n, sr, Syy, 5, 2, 25, fbase, df * scale, pbase, dphi * scale, f_min, f_max, red);
        if (r.R < R0) {
            R0 = r.R;
            fit_decode(r.c, 5, 2, fbase, df * scale, pbase, dphi * scale, f_min, f_max, f0, phi0);
        }
    }
}
