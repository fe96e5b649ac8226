// phaser_common.h -- what the phaser kernels (phaser.hip) and the adjoint (phaser_bwd.hip) share: the chunking of a clip, the
// per-clip constants, the cut-off update, the all-pass cascade and the layout of the stash that mx_phaser_fwd_stash leaves
// for mx_phaser_bwd.  The adjoint recomputes the forward bit for bit, so each of these is defined here once.
#pragma once
#include "common.h"

#define PS_WAVES 8
#define PS_P (64 * PS_WAVES)       // chunks (lanes) per clip
#define PS_MV 57                   // floats per chunk map: M column-major (49) + v (7) + pad
#define PS_LDS_FLOATS (PS_P * PS_MV + (PS_P + 1) * 8)
#define PS_SUB 2                   // cut-off groups (of 4 samples) between two state checkpoints of the stash (a power of two)

// Stash row of one clip, `sg` = stash_groups (a multiple of 4, >= the clip's cut-off groups), in floats:
//   [0, sg) G   [sg, 2 sg) pre = osc depth / 2 + norm_centre (before its clamp)   [2 sg, 3 sg) osc
//   [3 sg, 4 sg) int32: bit j set where sample 4 g + j passed the output clip (-1 <= m <= 1)
//   then PS_P chunk maps of PS_MV floats (the scan's M, column-major, + v), then the state checkpoints: 8 floats
//   (s0..s5, lastOut, pad) at the start of every PS_SUB-th group of every chunk, chunk p's at (p * spc + i) * 8 with
//   spc = ceil(groups per chunk / PS_SUB) of THAT clip.
__host__ __device__ inline long long ps_ckpts_per_chunk(long long n_groups)
{
    const long long gpc = (n_groups + PS_P - 1) / PS_P;
    return (gpc + PS_SUB - 1) / PS_SUB;
}
__host__ __device__ inline long long ps_stash_floats(long long sg)
{
    return 4 * sg + (long long)PS_P * PS_MV + (long long)PS_P * 8 * ps_ckpts_per_chunk(sg);
}

// The sections of a stash row.  F = float where the scan writes them, const float where the adjoint reads them.
__device__ __forceinline__ int *ps_as_int(float *p) { return reinterpret_cast<int *>(p); }
__device__ __forceinline__ const int *ps_as_int(const float *p) { return reinterpret_cast<const int *>(p); }
__device__ __forceinline__ float4 *ps_as_float4(float *p) { return reinterpret_cast<float4 *>(p); }
__device__ __forceinline__ const float4 *ps_as_float4(const float *p) { return reinterpret_cast<const float4 *>(p); }
template <typename F>
struct PsStash {
    F *row;
    int sg;
    __device__ __forceinline__ F *G() const { return row; }
    __device__ __forceinline__ F *pre() const { return row + sg; }
    __device__ __forceinline__ F *osc() const { return row + 2 * (size_t)sg; }
    __device__ __forceinline__ auto pass() const { return ps_as_int(row) + 3 * (size_t)sg; }
    __device__ __forceinline__ F *maps() const { return row + 4 * (size_t)sg; }
    // the two float4 of checkpoint `sub` of chunk p, in a clip of gpc groups per chunk
    __device__ __forceinline__ auto ckpt(int p, int gpc, int sub) const
    {
        return ps_as_float4(maps() + PS_P * PS_MV) + 2 * ((size_t)p * ((gpc + PS_SUB - 1) / PS_SUB) + sub);
    }
};

// ---- the arithmetic (oracle_ref.c:orc_phaser = JUCE dsp::Phaser<float>), fp32 in JUCE's operation order ------------------
constexpr float PS_TWO_PI = 6.283185307179586476925286766559f;
constexpr double PS_PI = 3.14159265358979323846;

// Per-clip constants.  inc: the LFO phase step per cut-off update (4 samples); span = log_max - log_min of the cut-off range.
struct PsClip {
    double sr;
    float log_min, span, inc, norm_centre, osc_vol, fb, wet_g, dry_g;
};
__device__ __forceinline__ PsClip ps_clip(double sr, float rate, float depth, float centre, float feedback, float mix)
{
    PsClip k;
    const float fmax_hz = (float)fmin(20000.0, 0.49 * sr);
    k.sr = sr;
    k.log_min = (float)log10(20.0);
    k.span = __fsub_rn((float)log10((double)fmax_hz), k.log_min);
    k.inc = __fmul_rn(__fdiv_rn(PS_TWO_PI, (float)(sr / 4.0)), rate);
    k.norm_centre = __fdiv_rn(__fsub_rn((float)log10((double)centre), k.log_min), k.span);
    k.osc_vol = __fmul_rn(depth, 0.5f);
    k.fb = feedback;
    k.wet_g = mix;
    k.dry_g = __fsub_rn(1.0f, mix);
    return k;
}

// The LFO: one phase step per cut-off update, accumulated in fp32 exactly as JUCE does; the oscillator at `phase`; and one
// cut-off update from the oscillator's value: G of the next four samples; pre: the lfo before its clamp (the adjoint's
// gate).  sin / pow / tan in fp64 and rounded once = the host libm's float results.
__device__ __forceinline__ float ps_step(float p, float inc)
{
    p = __fadd_rn(p, inc);
    while (p >= PS_TWO_PI) p = __fsub_rn(p, PS_TWO_PI);
    return p;
}
__device__ __forceinline__ float ps_osc(float phase) { return (float)sin((double)__fsub_rn(phase, (float)PS_PI)); }
__device__ __forceinline__ float ps_cutoff(const PsClip &k, float osc, float &pre)
{
    pre = __fadd_rn(__fmul_rn(osc, k.osc_vol), k.norm_centre);
    const float lfo = pre < 0.0f ? 0.0f : (pre > 1.0f ? 1.0f : pre);
    const float fc = (float)pow(10.0, (double)__fadd_rn(__fmul_rn(lfo, k.span), k.log_min));
    const float g = (float)tan(PS_PI * (double)fc / k.sr);
    return __fdiv_rn(g, __fadd_rn(1.0f, g));
}

// One first-order all-pass stage (JUCE's FirstOrderTPTFilter step): state s, signal out.  Returns d = out - s from before
// the update, which the adjoint keeps.
__device__ __forceinline__ float ps_stage(float G, float &s, float &out)
{
    const float d = __fsub_rn(out, s);
    const float v = __fmul_rn(G, d);
    const float yk = __fadd_rn(v, s);
    s = __fadd_rn(v, yk);
    out = __fsub_rn(__fmul_rn(2.0f, yk), out);
    return d;
}
// One sample through the six stages and the feedback: z = (s0..s5, lastOut); returns the wet signal; d (optional): the six d_k.
__device__ __forceinline__ float ps_sample(float G, float fb, float in, float (&z)[7], float *d = nullptr)
{
    float out = __fsub_rn(in, z[6]);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float dk = ps_stage(G, z[k], out);
        if (d) d[k] = dk;
    }
    z[6] = __fmul_rn(out, fb);
    return out;
}
