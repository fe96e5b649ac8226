// fx_params_common.h -- what more than one translation unit needs of the learned effect parameters: the slot constants of
// the per-row vectors and the sigmoid / lin / log map onto a parameter's range with its derivative (fx_params.hip: one shared
// value per entry; fx_head.hip: one value per clip).  One definition, so that a head with zero weights writes the bits the
// shared scalars write.
#pragma once
#include "common.h"

#define FXP_MAX_ENTRIES 16
#define FXP_LFO_SCALE 0
#define FXP_MIN_DELAY 1
#define FXP_FEEDBACK 2
#define FXP_DEPTH 3
#define FXP_MIX 4
#define FXP_CENTRE 5
#define FXP_SLOTS 6
#define FXP_THREADS 256

struct FxpOut { float *v[FXP_SLOTS]; float *one_minus_mix; };

__device__ __forceinline__ double fxp_sigmoid(double z)
{
    if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
    const double e = exp(z);
    return e / (1.0 + e);
}
// the mapped value and its derivative with respect to raw
__device__ __forceinline__ double fxp_value(double raw, double gain, double lo, double hi, int is_log, double *dv)
{
    const double s = fxp_sigmoid(gain * raw);
    const double ds = gain * s * (1.0 - s);
    if (is_log) {
        const double l0 = log(lo), span = log(hi) - l0;
        const double v = exp(l0 + span * s);
        if (dv) *dv = v * span * ds;
        return v;
    }
    if (dv) *dv = (hi - lo) * ds;
    return lo + (hi - lo) * s;
}
