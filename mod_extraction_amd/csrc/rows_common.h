// rows_common.h -- what the kernels on "B rows of N floats, a row stride apart, starting at any 4-byte boundary" share
// (gain_match.hip, fir_match.hip, pair_align.hip, and in part fx_head.hip, lfo_stitch.hip): on the device the split of a
// run of floats by the 16-byte alignment of its leading pointer, on the host the argument checks of their entry points.
// One definition each.  The walks over a span (a stride of 256 vectors, one thread a vector, ...) and the size limits stay
// with each file.
#pragma once
#include "common.h"

// device --------------------------------------------------------------------------------------
// floats before the first 16-byte boundary at or after p (p 4-byte aligned): 0..3
__device__ __forceinline__ int rows_head(const void *p)
{
    return (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
}

// four floats at any 4-byte boundary: still one dwordx4 load
struct __attribute__((packed, aligned(4))) RowsUFloat4 { float x, y, z, w; };

// len floats from lead: a scalar head up to the first 16-byte boundary, nvec aligned float4s, a scalar tail (0..3 floats)
struct RowsSpan { int head, nvec, tail; };
__device__ __forceinline__ RowsSpan rows_span(const float *lead, int len)
{
    RowsSpan s;
    int head = rows_head(lead);
    s.head = head < len ? head : len;
    s.nvec = (len - s.head) >> 2;
    s.tail = len - s.head - 4 * s.nvec;
    return s;
}

// host ----------------------------------------------------------------------------------------
static inline int rows_check(const void *p, int64_t stride, int64_t B, int64_t N)
{
    return (!p || B < 1 || N < 1 || stride < N) ? MX_ERR_ARG : MX_OK;
}

struct RowsRange { uintptr_t lo, hi; };                           // the bytes [lo, hi)
static inline RowsRange rows_range(const void *p, int64_t stride, int64_t B, int64_t N)  // B rows of N floats, first to last element
{
    return {(uintptr_t)p, (uintptr_t)p + 4 * (uintptr_t)((B - 1) * stride + N)};
}
static inline RowsRange rows_flat(const void *p, int64_t count, int64_t elem)            // count elements of elem bytes
{
    return {(uintptr_t)p, (uintptr_t)p + (uintptr_t)(count * elem)};
}
static inline bool rows_overlap(RowsRange a, RowsRange b)
{
    return a.lo < b.hi && b.lo < a.hi;
}
// does one of the n_out output ranges share a byte with another output or with one of the n_in input ranges?
static inline bool rows_any_overlap(const RowsRange *out, int n_out, const RowsRange *in, int n_in)
{
    for (int i = 0; i < n_out; ++i) {
        for (int j = i + 1; j < n_out; ++j)
            if (rows_overlap(out[i], out[j])) return true;
        for (int j = 0; j < n_in; ++j)
            if (rows_overlap(out[i], in[j])) return true;
    }
    return false;
}
