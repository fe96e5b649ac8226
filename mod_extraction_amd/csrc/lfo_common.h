// lfo_common.h -- the LFO arithmetic more than one translation unit evaluates: the closed-form LFO value and its phase
// step (lfo.hip, lfo_variants.hip) and the corner rule (corners.hip, lfo_variants.hip).  One definition each, so that a
// label synthesised or searched for corners in one kernel has the bits of the other.
#pragma once
#include "common.h"

#define LFO_COS 0
#define LFO_RECT_COS 1
#define LFO_INV_RECT_COS 2
#define LFO_TRI 3
#define LFO_SAW 4
#define LFO_RSAW 5
#define LFO_SQR 6

// modulations.py:26-31: the rectified cosines run at half rate / half phase (exact halving, applied to f and ph in place);
// returns the fp32 phase step 2 pi f / sr.
__device__ __forceinline__ float lfo_step(int sh, float &f, float &ph, float sr)
{
    const float TWO_PI_F = 6.283185307179586f;
    if (sh == LFO_RECT_COS || sh == LFO_INV_RECT_COS) {  // modulations.py:26-29 (exact halving)
        f = __fmul_rn(f, 0.5f);
        ph = __fmul_rn(ph, 0.5f);
    }
    return __fdiv_rn(__fmul_rn(TWO_PI_F, f), sr);  // modulations.py:31
}

__device__ __forceinline__ float lfo_value(int k, int start, float step, float ph, int shape, float ex)
{
    const float TWO_PI_F = 6.283185307179586f;
    const float PI_F = 3.141592653589793f;
    const float HALF_PI_F = 1.5707963267948966f;
    double run = (double)((long long)k + 1 + (long long)start) * (double)step;
    float arg = __fadd_rn(__double2float_rn(run), ph);
    float v;
    if (shape == LFO_COS) {
        v = __fmul_rn(__fadd_rn(cosf(__fadd_rn(arg, PI_F)), 1.0f), 0.5f);
    } else if (shape == LFO_RECT_COS) {
        v = fabsf(cosf(__fadd_rn(arg, HALF_PI_F)));
    } else if (shape == LFO_INV_RECT_COS) {
        v = __fadd_rn(-fabsf(cosf(arg)), 1.0f);
    } else if (shape == LFO_SQR) {
        float c = cosf(__fadd_rn(arg, PI_F));
        float s = c > 0.0f ? 1.0f : (c < 0.0f ? -1.0f : 0.0f);
        v = __fmul_rn(__fadd_rn(s, 1.0f), 0.5f);
    } else {
        float saw = __fdiv_rn(torch_remainderf(arg, TWO_PI_F), TWO_PI_F);
        if (shape == LFO_SAW) {
            v = saw;
        } else if (shape == LFO_RSAW) {
            v = __fsub_rn(1.0f, saw);
        } else {  // LFO_TRI
            float tri = __fmul_rn(2.0f, saw);
            v = tri > 1.0f ? __fsub_rn(2.0f, tri) : tri;
        }
    }
    if (ex != 1.0f) {
        // torch.pow(tensor, scalar) fast paths (aten PowKernel.cpp), then the generic powf
        if (ex == 2.0f) v = __fmul_rn(v, v);
        else if (ex == 3.0f) v = __fmul_rn(__fmul_rn(v, v), v);
        else if (ex == 0.5f) v = sqrtf(v);
        else v = powf(v, ex);
    }
    return v;
}

// top/bottom corner value at interior index i (modulations.py:224-231):
//   -floor( (d_l > 0 ? d_l : 0) * (d_r + 1e-16) )  and the same with d_l < 0
__device__ __forceinline__ void corner_values(const float *m, int i, float &top, float &bot)
{
    const float d_l = __fsub_rn(m[i], m[i - 1]);
    const float d_r = __fsub_rn(m[i + 1], m[i]);
    const float nudged = __fadd_rn(d_r, 1e-16f);
    const float rising = d_l > 0.0f ? d_l : 0.0f;
    const float falling = d_l < 0.0f ? d_l : 0.0f;
    top = (float)(-(long long)floorf(__fmul_rn(rising, nudged)));
    bot = (float)(-(long long)floorf(__fmul_rn(falling, nudged)));
}
