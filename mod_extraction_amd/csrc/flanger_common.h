// flanger_common.h -- what the flanger / chorus forward (flanger.hip) and its adjoint (flanger_bwd.hip) share: the chunk and
// ring geometry, the fp32 index bookkeeping of fx.py:95-103, the slot word of a record and the dependency-free runs of a
// row.  The adjoint must reproduce the forward's slots and runs bit for bit, so each of them is defined here once.
#pragma once
#include "common.h"

#define FL_V 8                 // rows of 64 samples per chunk (4: 0.58 of the independent floor on config 3, 6: 0.60, 8: 0.62 -- the per-chunk barrier and the consumer's record loads amortise over more rows; 12 would need 132 consumer registers)
#define FL_CHUNK (64 * FL_V)
#define FL_SLOT_FLOATS (FL_CHUNK * 6 + 2 * FL_V)          // FL_CHUNK float4 records, FL_CHUNK 64-bit lane masks (run r of a row in lane r), FL_V run counts
#define FL_RING_FLOATS (2 * FL_SLOT_FLOATS)
#define FL_MAX_M (40960 - FL_RING_FLOATS)                // 160 KB LDS = 40960 floats, minus the ring
#define FL_THREADS (64 * (1 + FL_V))   // consumer wave + one producer wave per row of a chunk

// the three sections of ring slot c & 1 (the producers fill the slot of one chunk while the consumer reads the other)
struct FlSlot { float4 *rec; unsigned long long *run_mask; int *n_runs; };
__device__ __forceinline__ FlSlot fl_slot(float *ring, int c)
{
    float *s = ring + (c & 1) * FL_SLOT_FLOATS;
    return {reinterpret_cast<float4 *>(s), reinterpret_cast<unsigned long long *>(s + 4 * FL_CHUNK),
            reinterpret_cast<int *>(s + 6 * FL_CHUNK)};
}

// fx.py:95-103 for one sample with write slot w = n % M and LFO value m, in exactly the reference's rounding sequence (fp32,
// no contraction): read slots prev / next and the read fraction.
__device__ __forceinline__ void fl_slots(int w, float m, float ls, float md, int M, float Mf, int &prev, int &next,
                                         float &frac)
{
    const float d = __fadd_rn(__fmul_rn(ls, m), md);                    // fx.py:99
    const float r1 = __fadd_rn(__fsub_rn((float)w, d), Mf);             // fx.py:100
    float r;
    if (r1 >= 0.0f && r1 < Mf) r = r1;                                  // fmod is the identity here
    else if (r1 >= Mf && r1 < __fadd_rn(Mf, Mf)) r = __fsub_rn(r1, Mf); // exact (Sterbenz)
    else r = torch_remainderf(r1, Mf);                                  // out-of-contract mod_sig: generic path
    const float fl = floorf(r);
    int p = (int)fl;                                                    // fx.py:102
    if (p < 0) p = 0;                                                   // NaN / garbage guard (never hit in contract)
    if (p >= M) p = M - 1;
    prev = p;
    next = p + 1 == M ? 0 : p + 1;                                      // fx.py:103
    frac = __fsub_rn(r, fl);                                            // fx.py:101
}

// The LFO value of sample n from a row of n_mod < N points (util.py:15-29, align_corners=True; scale =
// interp_scale_host(n_mod, N)): the taps of interp_tap and their combination, one definition for the forward's producers
// and for both adjoint kernels, so that the m -- and with it the slots, fractions and runs -- of a sample agree bit for bit.
__device__ __forceinline__ float fl_lfo(const float *row, float scale, int n, int n_mod)
{
    const InterpTap t = interp_tap(scale, n, n_mod);
    return interp_combine(t, row[t.i0], row[t.i1]);
}

// distance back from the write at slot w to the last write of slot s (slot w itself is "M samples ago")
__device__ __forceinline__ int fl_dist(int w, int s, int M)
{
    const int d = w - s;
    return d <= 0 ? d + M : d;
}

// the slot word of a record: w | prev << 16 (M < 65536, checked by the launchers); next follows from prev (fx.py:103)
__device__ __forceinline__ float fl_pack(int w, int prev) { return __int_as_float(w | (prev << 16)); }
__device__ __forceinline__ void fl_unpack(float word, int M, int &w, int &prev, int &next)
{
    const int pk = __float_as_int(word);
    w = pk & 0xffff;
    prev = (pk >> 16) & 0xffff;
    next = prev + 1 == M ? 0 : prev + 1;
}

// Maximal dependency-free runs of a row of 64 samples.  tk: the newest sample of the row this lane's sample depends on (-1:
// none); the run starting at a ends in front of the first k >= a with tk[k] >= a.  tk < lane, so every run is non-empty.
// Lane r receives the lane mask of run r (lanes [a, bnd) as a 64-bit exec image, restricted to `live`): the consumer
// fetches a step's mask with two v_readlane instead of deriving it.  n_runs: the number of runs (wave-uniform).
__device__ __forceinline__ unsigned long long fl_run_masks(int lane, int tk, unsigned long long live, int &n_runs)
{
    unsigned long long mine = 0ull;
    int a = 0, run = 0;
    while (a < 64) {
        const unsigned long long conflict = __ballot(lane >= a && tk >= a);
        const int bnd = conflict ? (int)__builtin_ctzll(conflict) : 64;
        if (lane == run) mine = (~0ull << a) & (~0ull >> (64 - bnd)) & live;
        a = bnd;
        ++run;
    }
    n_runs = run;
    return mine;
}
