// spectral_pair.h -- the packed two-signal frame of the spectral losses: one complex transform of x + i y per frame (wave_fft.h)
// carries a prediction frame and its target frame; these helpers load such a frame, equalise the two levels before packing
// and detect frames whose spectra are equal by construction.  Users: the MR-STFT loss (mrstft.hip, mod_extraction/losses.py:
// 155-156) and the log-mel L1 loss (logmel_loss.hip, mod_extraction/losses.py:105-130).
#pragma once
#include "wave_fft.h"

__device__ __forceinline__ int reflect_index(int s, int T)
{
    if (s < 0) s = -s;
    if (s >= T) s = 2 * (T - 1) - s;
    return s;
}

// frame f of x + i*y, centre / reflect padded, UNWINDOWED, straight into the stage-A register layout (the one-pass kernels
// fetch a frame while the frame before it is transformed).  INTERIOR (wave-uniform): no position of the frame needs the
// reflection arithmetic, the loads are one base pointer + constant offsets.
template <int N, bool INTERIOR>
__device__ __forceinline__ void fetch_frame(cf (&R)[WF<N>::NB][4], const float *xb, const float *yb, int f, int hop, int T, int a)
{
    const float *xf = xb + (f * hop - N / 2 + a), *yf = yb + (f * hop - N / 2 + a);     // dereferenced only when INTERIOR
#pragma unroll
    for (int b = 0; b < WF<N>::NB; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (INTERIOR) {
                R[b][c] = {xf[WF<N>::L * b + (N / 4) * c], yf[WF<N>::L * b + (N / 4) * c]};
            } else {
                const int s = reflect_index(f * hop + a + WF<N>::L * b + (N / 4) * c - N / 2, T);
                R[b][c] = {xb[s], yb[s]};
            }
        }
}

// sum over the L lanes of a frame (the whole wave; a half for 512), the same value on every lane of the frame: within each row
// of 16 lanes by DPP (lane xor 1, xor 2, mirror within 8, mirror within 16 -- each step adds two operands that the partner lane
// adds in the other order), then the row sums by v_readlane (no LDS round trip on the path into the transform)
template <int L>
__device__ __forceinline__ float frame_sum(float v)
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));     // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));     // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));    // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));    // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    if (L == 64) return (r0 + r1) + (r2 + r3);
    return (threadIdx.x & 32) ? r2 + r3 : r0 + r1;
}

// (sum x_w^2, sum y_w^2) of the lane's frame, on every lane of the frame
template <int N>
__device__ __forceinline__ cf frame_energy(const cf (&R)[WF<N>::NB][4])
{
    cf e = {0.0f, 0.0f};
#pragma unroll
    for (int bq = 0; bq < WF<N>::NB; ++bq)
#pragma unroll
        for (int c = 0; c < 4; ++c) asm("v_pk_fma_f32 %0, %1, %1, %0" : "+v"(e) : "v"(R[bq][c]));
    return {frame_sum<WF<N>::L>(e.x), frame_sum<WF<N>::L>(e.y)};
}

// A frame whose windowed signals are bit-identical (x == y) or bit-negated (x == -y) has |X| == |Y| bin for bin in the
// reference (the transform of -y is the negated transform of y): keep that exact (loss 0, gradient 0), where the packed
// transform's split would leave |X| != |Y| at rounding level.  Taken on the UNSCALED windowed frame (before pack_gain).  Such a
// frame has e.x == e.y exactly (the same squares summed in the same order), so the element-wise test runs only then.
template <int N>
__device__ __forceinline__ bool frame_same(const cf (&R)[WF<N>::NB][4], int g, cf e)
{
    const bool level = e.x == e.y;                            // the same on every lane of the frame
    if (__ballot(level) == 0ull) return false;
    bool eq = true, neg = true;
#pragma unroll
    for (int bq = 0; bq < WF<N>::NB; ++bq)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            eq = eq && R[bq][c].x == R[bq][c].y;
            neg = neg && R[bq][c].x == -R[bq][c].y;
        }
    const unsigned long long me = __ballot(eq), mn = __ballot(neg);
    if (WF<N>::L == 64) return level && (me == ~0ull || mn == ~0ull);
    const unsigned long long h = 0xffffffffull << (32 * g);
    return level && ((me & h) == h || (mn & h) == h);
}

// Level equalisation of the packed pair.  Separating the two spectra from ONE transform of x + i y leaves an error of about
// u ||louder windowed frame|| on BOTH spectra, which on the quieter signal's bins can be large relative to the bins (and the
// log term and its 1 / |X| gradient amplify it).  So the target frame is packed as s y, s = 2^k, k = round(log2(||x_w|| /
// ||y_w||)) clamped to [-60, 60] (0 when |k| < 2, when either frame is all zeros, or for a `same` frame): both halves carry the same
// level and each spectrum gets the error of its own transform.  A power of two scales exactly, so |Y|^2 = |D|^2 s^-2 with
// nothing lost; the return value is s^-2.  e: frame_energy of the unscaled frame.
template <int N>
__device__ __forceinline__ float pack_gain(cf (&R)[WF<N>::NB][4], bool same, cf e)
{
    const float ex = e.x, ey = e.y;
    float kf = 0.5f * (__builtin_amdgcn_logf(ex) - __builtin_amdgcn_logf(ey));
    kf = fminf(fmaxf(rintf(kf), -60.0f), 60.0f);              // (fmaxf drops a NaN of inf - inf)
    // k = +-1 is left at 0: a level difference below ~2.8x costs the quieter spectrum at most that factor, and frames at
    // comparable levels (a prediction close to its target) keep the arithmetic, and the rounding, of the unscaled pack
    const int k = (same || !(ex > 0.0f) || !(ey > 0.0f) || fabsf(kf) < 2.0f) ? 0 : (int)kf;
    if (k == 0) return 1.0f;
    const float s = ldexpf(1.0f, k);
#pragma unroll
    for (int bq = 0; bq < WF<N>::NB; ++bq)
#pragma unroll
        for (int c = 0; c < 4; ++c) R[bq][c].y *= s;
    return ldexpf(1.0f, -2 * k);
}

// packed-fp32 helpers of the Hermitian separation / completion
__device__ __forceinline__ cf add_conj(cf a, cf b)          // (a.x + b.x, a.y - b.y)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ cf sub_conj(cf a, cf b)          // (a.x - b.x, a.y + b.y)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ cf mirror_h(cf ga, cf gb)        // conj(ga) + i conj(gb) = (ga.x + gb.y, gb.x - ga.y)
{
    cf r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[1,0]" : "=v"(r) : "v"(ga), "v"(gb));
    return r;
}
