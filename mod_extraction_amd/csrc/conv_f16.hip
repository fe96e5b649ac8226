// conv_f16.hip -- the 64->64 channel Spectral2DCNN convolutions (forward and data gradient) on the
// fp16 matrix cores with fp32-equivalent accuracy ("f16x3" split arithmetic).
// Reference semantics are unchanged: mod_extraction/models.py:183-195, LayerNorm -> Conv2d(5x13,
// dilation (1,T), same) -> +bias -> MaxPool(2,1), and the conv's data gradient.
//
// Why: v_mfma_f32_32x32x2_f32 runs at 157 TFLOP/s, v_mfma_f32_32x32x16_f16 at 16x that rate.  Every fp32
// operand x is split once into two fp16 numbers, x*S ~= hi + lo (hi = fp16(x*S), lo = fp16(x*S - hi),
// S a power of two), and the product of two fp32 numbers is evaluated as hi*hi + hi*lo + lo*hi -- three
// fp16 MFMAs accumulating in fp32.  hi+lo carries 22 mantissa bits, the dropped lo*lo term is 2^-22
// relative: measured end to end (6 blocks) the sigmoid output / latent differ from an fp64 evaluation
// by 4e-7 / 2.4e-6, the same as true fp32 arithmetic (4.9e-7 / 3.1e-6) and well inside the 1e-5 gate.
// Three MFMAs per fp32 MAC group = 5.3x the fp32-MFMA rate.
//
// Operands are prepared once per layer by streaming kernels in channels-last fp16 pairs
//   X_hi, X_lo : (B, H, 4, 352, 16)  forward: (prelu(p_prev) - mean) * rstd        (S = 1)
//                                    dgrad  : max-pool routed gradient * S_dz      (S_dz = 2^k from max|G|)
//                channel-block major: a K stage consumes ONE 16-channel block of a row, which is then a contiguous
//                11 KB run of full cache lines (with the 64 channels of a position adjacent, every stage would touch
//                a quarter of each line of the row and the row would be pulled from HBM once per block: measured 16x
//                the algorithmic traffic)
//   W_hi, W_lo : [ci/16][kh][kw][khalf][co][8]  weights * 256 (pack_weights_f16_kernel)
// so that the conv kernel stages plain 16-byte vectors and every MFMA fragment (8 consecutive channels of
// one position / one output channel) is ONE aligned ds_read_b128.
//
// Kernel: one 256-thread workgroup per (clip, output-row pair), 1 workgroup per CU (LDS 100-155 KB,
// <= 512 VGPRs per wave).  K loop = 4 channel blocks x 5 kernel rows = 20 stages; per stage the 13 taps of
// one kernel row for 16 input channels: weights 53 KB + the two needed input rows (46-51 KB) in LDS.
// The next stage's global loads are issued into registers before the current stage's MFMAs (26 vectors per
// thread), fragments are software pipelined in two half-tap sets.  4 waves = (co tile) x (output row),
// 11 accumulators of 32x32 each; epilogue identical to the fp32 kernel (bias + max-pool + argmax, or plain).
// That kernel (conv_f16x3_kernel, operands staged through registers) still runs the DENSE data gradient at dilation 8 and
// 16.  The forward runs on its LDS-DMA descendants below: conv_f16x3_dma16_kernel (dilation <= 4, four-row patch ring),
// conv_f16x3_dma3_kernel (dilation 8 and 16, three-row patch ring, halo tiles left out), conv1_f16x3_tile_kernel (first
// block); the dense data gradient at dilation <= 4 on conv_f16x3_dma_kernel.
#include "conv_common.h"
#include <hip/hip_fp16.h>
#include <type_traits>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
#define F16_WSCALE 256.0f

__device__ __forceinline__ floatx16 mfma16(half8 a, half8 b, floatx16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// ---- operand preparation -----------------------------------------------------------------------------
// scale[0] = S (power of two with max|x| * S in [512, 1024)), scale[1] = 1 / S; amax_bits = bit pattern of max|x|
// (over the Wv valid columns of the 352-float rows only: what the pad columns hold must not reach the scale)
__global__ void absmax_kernel(const float *__restrict__ x, long long n4, int Wv, unsigned *__restrict__ amax_bits)
{
    float m = 0.0f;
    const floatx4 *p = reinterpret_cast<const floatx4 *>(x);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        floatx4 v = p[i];
        const int w0 = (int)(i % (CV_PITCH / 4)) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, w0 + e < Wv ? fabsf(v[e]) : 0.0f);
    }
    m = wave_max_f32(m);
    if ((threadIdx.x & 63) == 0) atomicMax(amax_bits, __float_as_uint(m));   // order of non-negative floats = order of bits
}
__global__ void pow2_scale_kernel(const unsigned *__restrict__ amax_bits, float *__restrict__ scale)
{
    const float m = __uint_as_float(*amax_bits);
    int e = 0;
    if (m > 0.0f && m < 3.0e38f) {
        frexpf(m, &e);                 // m = f * 2^e, f in [0.5, 1)
        e = 10 - e;                    // m * 2^(10 - e) in [512, 1024)
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
    }
    scale[0] = ldexpf(1.0f, e);
    scale[1] = ldexpf(1.0f, -e);
}

// NCHW fp32 planes -> channels-last fp16 pairs.  One workgroup per (b, h, 32-column tile): 64 channels x
// 32 columns are read along w (coalesced), transformed, transposed through LDS and written as 16-byte
// vectors of 8 channels into the (B, H, 4, 352, 16) operand (1 KB contiguous per channel block).  MODE 0: xhat = (prelu(x) - mean) * rstd.  MODE 1: dz = routed G * S.
// Forward operand (MODE 0 of split_prep_kernel) with ROWS image rows per workgroup: all of a thread's 2 * ROWS 16-byte
// loads are in flight together (the one-row kernel had 2), and the transposing LDS pass is amortised over more bytes.
template <int ROWS>
__global__ __launch_bounds__(256) void split_prep_fwd_kernel(const float *__restrict__ x, const float *__restrict__ stats,
                                                             const float *__restrict__ slope, int H, int Wv,
                                                             _Float16 *__restrict__ out_hi, _Float16 *__restrict__ out_lo)
{
    __shared__ float tile[ROWS][64][33];
    const int wt = blockIdx.x, h0 = blockIdx.y * ROWS, b = blockIdx.z, tid = threadIdx.x;
    floatx4 v[ROWS][2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + 256 * k, c = i >> 3, c4 = i & 7;
        const size_t off = (((size_t)b * 64 + c) * H + h0) * CV_PITCH + wt * 32 + c4 * 4;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) v[r][k] = __builtin_nontemporal_load(reinterpret_cast<const floatx4 *>(x + off + (size_t)r * CV_PITCH));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + 256 * k, c = i >> 3, c4 = i & 7, w0 = wt * 32 + c4 * 4;
        const float mean = stats[((size_t)b * 64 + c) * 2], rstd = stats[((size_t)b * 64 + c) * 2 + 1], sl = slope[c];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = v[r][k][e] > 0.0f ? v[r][k][e] : sl * v[r][k][e];
                tile[r][c][c4 * 4 + e] = (w0 + e < Wv) ? (t - mean) * rstd : 0.0f;
            }
    }
    __syncthreads();
    const int pos = tid >> 3, cg = tid & 7;                     // 32 positions x 64 channels: thread -> (position, 8 channels)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        half8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = tile[r][cg * 8 + j][pos];
            const _Float16 hh = (_Float16)t;
            hi[j] = hh;
            lo[j] = (_Float16)(t - (float)hh);
        }
        const size_t o = ((((size_t)b * H + h0 + r) * 4 + (cg >> 1)) * CV_PITCH + wt * 32 + pos) * 16 + (cg & 1) * 8;
        __builtin_nontemporal_store(hi, reinterpret_cast<half8 *>(out_hi + o));
        __builtin_nontemporal_store(lo, reinterpret_cast<half8 *>(out_lo + o));
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void split_prep_kernel(const float *__restrict__ x,
                                                         const unsigned char *__restrict__ amax,
                                                         const float *__restrict__ stats,
                                                         const float *__restrict__ slope,
                                                         const float *__restrict__ scale, int H, int Wv,
                                                         _Float16 *__restrict__ out_hi, _Float16 *__restrict__ out_lo)
{
    __shared__ float tile[64][33];
    const int wt = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int Hin = MODE == 1 ? (H >> 1) : H, hin = MODE == 1 ? (h >> 1) : h;
    const float S = MODE == 1 ? scale[0] : 1.0f;
    for (int i = tid; i < 64 * 8; i += 256) {
        const int c = i >> 3, c4 = i & 7;
        const int w0 = wt * 32 + c4 * 4;
        const size_t off = (((size_t)b * 64 + c) * Hin + hin) * CV_PITCH + w0;
        floatx4 v = *reinterpret_cast<const floatx4 *>(x + off);
        if (MODE == 1) {
            const uchar4 am = *reinterpret_cast<const uchar4 *>(amax + off);
            const unsigned want = (unsigned)(h & 1);
            v[0] = am.x == want ? v[0] * S : 0.0f;
            v[1] = am.y == want ? v[1] * S : 0.0f;
            v[2] = am.z == want ? v[2] * S : 0.0f;
            v[3] = am.w == want ? v[3] * S : 0.0f;
        } else {
            const float mean = stats[((size_t)b * 64 + c) * 2], rstd = stats[((size_t)b * 64 + c) * 2 + 1], sl = slope[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = v[e] > 0.0f ? v[e] : sl * v[e];
                v[e] = (t - mean) * rstd;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[c][c4 * 4 + e] = (w0 + e < Wv) ? v[e] : 0.0f;
    }
    __syncthreads();
    // 32 positions x 64 channels: thread -> (position, 8-channel group)
    const int pos = tid >> 3, cg = tid & 7;
    half8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = tile[cg * 8 + j][pos];
        const _Float16 hh = (_Float16)v;
        hi[j] = hh;
        lo[j] = (_Float16)(v - (float)hh);
    }
    const size_t o = ((((size_t)b * H + h) * 4 + (cg >> 1)) * CV_PITCH + wt * 32 + pos) * 16 + (cg & 1) * 8;
    *reinterpret_cast<half8 *>(out_hi + o) = hi;
    *reinterpret_cast<half8 *>(out_lo + o) = lo;
}

// torch (64, 64, 5, 13) fp32 -> [ci/16][kh][kw][khalf][co][8] fp16 pairs of W * 256 (the LDS image of a stage, so
// that staging is a linear copy: the two 8-channel halves of a 16-channel block are separate planes)
//   flip = 0 (forward): in = ci, out = co;  flip = 1 (dgrad): in = co, out = ci, taps mirrored
__global__ void pack_weights_f16_kernel(const float *__restrict__ W, int flip, _Float16 *__restrict__ w_hi,
                                        _Float16 *__restrict__ w_lo)
{
    const int total = 64 * 64 * CV_TAPS;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int kw = i % CV_KW, kh = (i / CV_KW) % CV_KH, ci = (i / CV_TAPS) % 64, co = i / (CV_TAPS * 64);
        const float v = W[i] * F16_WSCALE;
        const _Float16 hh = (_Float16)v;
        const _Float16 ll = (_Float16)(v - (float)hh);
        int cin, cout, kh2, kw2;
        if (!flip) { cin = ci; cout = co; kh2 = kh; kw2 = kw; }
        else { cin = co; cout = ci; kh2 = CV_KH - 1 - kh; kw2 = CV_KW - 1 - kw; }
        const size_t o = (((((size_t)(cin >> 4) * CV_KH + kh2) * CV_KW + kw2) * 2 + ((cin & 15) >> 3)) * 64 + cout) * 8 + (cin & 7);
        w_hi[o] = hh;
        w_lo[o] = ll;
    }
}

// ---- first block (2 input channels): the operand carries (kernel row, channel) as its 16 "channels" ---------------
// x (B, 2, H, 352) fp32 log-mel, stats (B, 2, 2) -> xk_hi, xk_lo (B, H, 1, 352, 16): channel k = kh * 2 + ci (k < 10)
// holds xhat[ci][h + kh - 2][w] = (x - mean) * rstd (0 outside the image), k >= 10 is 0.  One 16-deep MFMA k-step then
// covers a whole tap COLUMN of the 5x13 kernel for both channels, and the K loop of the conv kernel is a single stage.
// One workgroup = KV_ROWS consecutive output rows of a clip over the full width: the KV_ROWS + 4 input rows of both channels
// are read ONCE (coalesced 16-byte loads), normalised into LDS, and every thread writes whole 16-byte vectors of the pair
// (the first version -- 32 columns of one row per workgroup, 128 of 256 threads loading, 64 storing, every input row read five
// times -- ran at a third of the HBM rate: 0.76 ms per 256 clips for 1.5 GB of output; this one 0.38 ms; 4 / 16 rows per workgroup: 0.52 / 0.46).
#define KV_ROWS 8
__global__ __launch_bounds__(256) void split_prep_kvec_kernel(const float *__restrict__ x, const float *__restrict__ stats,
                                                              int H, int Wv, _Float16 *__restrict__ out_hi,
                                                              _Float16 *__restrict__ out_lo)
{
    constexpr int NR = (KV_ROWS + 4) * 2, RS = CV_PITCH + 1;       // (input row, channel) images; odd stride: the 8 rows a thread reads fall in 8 banks
    __shared__ float tile[NR * RS];
    const int h0 = blockIdx.x * KV_ROWS, b = blockIdx.y, tid = threadIdx.x;
    float mean[2], rstd[2];
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) { mean[ci] = stats[((size_t)b * 2 + ci) * 2]; rstd[ci] = stats[((size_t)b * 2 + ci) * 2 + 1]; }
    for (int i = tid; i < NR * (CV_PITCH / 4); i += 256) {
        const int rw = i / (CV_PITCH / 4), c4 = i - rw * (CV_PITCH / 4), ci = rw & 1, hx = h0 - 2 + (rw >> 1), w0 = c4 * 4;
        floatx4 v = {0.f, 0.f, 0.f, 0.f};
        if (hx >= 0 && hx < H) {
            v = *reinterpret_cast<const floatx4 *>(x + (((size_t)b * 2 + ci) * H + hx) * CV_PITCH + w0);
            const float m = ci ? mean[1] : mean[0], r = ci ? rstd[1] : rstd[0];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (w0 + e < Wv) ? (v[e] - m) * r : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[rw * RS + w0 + e] = v[e];
    }
    __syncthreads();
    for (int i = tid; i < KV_ROWS * CV_PITCH * 2; i += 256) {       // (output row, position, group of 8 channels)
        const int r = i / (CV_PITCH * 2), rem = i - r * (CV_PITCH * 2), pos = rem >> 1, cg = rem & 1, h = h0 + r;
        if (h >= H) break;
        half8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = cg * 8 + j;                               // channel k = kh * 2 + ci: image (r + kh) * 2 + ci = 2 r + k
            const float v = k < 2 * CV_KH ? tile[(2 * r + k) * RS + pos] : 0.0f;
            const _Float16 hh = (_Float16)v;
            hi[j] = hh;
            lo[j] = (_Float16)(v - (float)hh);
        }
        const size_t o = (((size_t)b * H + h) * CV_PITCH + pos) * 16 + cg * 8;
        __builtin_nontemporal_store(hi, reinterpret_cast<half8 *>(out_hi + o));
        __builtin_nontemporal_store(lo, reinterpret_cast<half8 *>(out_lo + o));
    }
}

// torch (64, 2, 5, 13) fp32 -> [kw][khalf][co][8] fp16 pairs of W * 256 with k = kh * 2 + ci (zeros for k >= 10)
__global__ void pack_weights_kvec_f16_kernel(const float *__restrict__ W, _Float16 *__restrict__ w_hi,
                                             _Float16 *__restrict__ w_lo)
{
    const int total = CV_KW * 2 * 64 * 8;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int j = i & 7, co = (i >> 3) & 63, khalf = (i >> 9) & 1, kw = i >> 10;
        const int k = khalf * 8 + j, kh = k >> 1, ci = k & 1;
        float v = 0.0f;
        if (k < 2 * CV_KH) v = W[(((size_t)co * 2 + ci) * CV_KH + kh) * CV_KW + kw] * F16_WSCALE;
        const _Float16 hh = (_Float16)v;
        w_hi[i] = hh;
        w_lo[i] = (_Float16)(v - (float)hh);
    }
}

// ---- the convolution ------------------------------------------------------------------------------------
struct ConvF16Args {
    const _Float16 *x_hi, *x_lo;   // (B, H, 4, 352, 16)
    const _Float16 *w_hi, *w_lo;   // [4][5][13][2][64][8]
    const float *bias;             // forward: (64,)
    const float *scale;            // dgrad: {S_dz, 1/S_dz} on the device; forward: nullptr
    float *out;                    // forward: (B, 64, H/2, 352) pooled pre-activations; dgrad: (B, 64, H, 352)
    unsigned char *out_amax;       // forward
    int H, Wv;
    // forward, optional: the LayerNorm statistics of the NEXT block are those of PReLU(out) per (clip, channel) plane; with
    // slope_out (64,) the epilogue leaves {sum, sum of squares} of PReLU(out) - PReLU(bias) per (clip, pooled row, channel) in
    // stats_part (B, H/2, 64, 2) and mx_plane_stats_finish turns them into mean / rstd: the plane is never re-read (norm.hip
    // plane_stats_kernel swept 5.9 GB per step for them)
    const float *slope_out;
    float *stats_part;
};

// Epilogue shared by the conv kernels.  Wave = (output row, column half c); accumulator layout
//   acc[2t + j], t < 5 : column tile c*6 + t, channel half j ^ c;      acc[10] : column tile 5, channel half c
// OUTMODE 0: bias + max-pool over the row pair + argmax (rows exchanged through LDS), 1: plain rows * 1/S.
// logical 32 x 32 tile i of a wave's accumulators -> [32 co][32 w] fp32 image (4 KB)
//   floatx16[11] (v_mfma_f32_32x32x16_f16): tile i is acc[i]
//   floatx4[44]  (v_mfma_f32_16x16x32_f16): tile i < 10 = 16-column tiles 2 (i >> 1) + dn, channel tiles 2 (i & 1) + dm of
//                acc[nt * 4 + ct]; tile 10 = acc[40 + dn * 2 + dm]; element (lane, r): co = 4 (lane >> 4) + r, w = lane & 15
__device__ __forceinline__ void store_tile32(const floatx16 (&acc)[CV_WT], int i, float *dst, int lane)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[mfma_row(r, lane) * 32 + (lane & 31)] = acc[i][r];
}
__device__ __forceinline__ void store_tile32(const floatx4 (&acc)[44], int i, float *dst, int lane)
{
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int dm = 0; dm < 2; ++dm) {
            const int u = i < 10 ? (2 * (i >> 1) + dn) * 4 + 2 * (i & 1) + dm : 40 + dn * 2 + dm;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(dm * 16 + (lane >> 4) * 4 + r) * 32 + dn * 16 + (lane & 15)] = acc[u][r];
        }
}
__device__ __forceinline__ float acc_elem(const floatx16 (&acc)[CV_WT], int i, int r) { return acc[i][r]; }
__device__ __forceinline__ float acc_elem(const floatx4 (&acc)[44], int, int) { return 0.0f; }      // (plain rows: 32x32 layout only)

template <int OUTMODE, typename ACC>
__device__ __forceinline__ void conv_f16_epilogue(ACC &acc, const ConvF16Args &a, unsigned char *smem,
                                                  int b, int h0, int row, int c, int lane)
{
    const int l32 = lane & 31;
    // ---- epilogue (same data layout as the fp32 kernel) ----
    const float inv = (OUTMODE == 1 ? a.scale[1] : 1.0f) * (1.0f / F16_WSCALE);
    if (OUTMODE == 1) {
        const int h = h0 + row;
#pragma unroll
        for (int i = 0; i < CV_WT; ++i) {
            const int w = (i == 10 ? 5 : c * 6 + (i >> 1)) * 32 + l32;
            const int cb0 = (i == 10 ? c : (i & 1) ^ c) * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb0 + mfma_row(r, lane);
                a.out[(((size_t)b * CV_CO + co) * a.H + h) * CV_PITCH + w] = w < a.Wv ? acc_elem(acc, i, r) * inv : 0.0f;
            }
        }
    } else {
        // Max-pool over the row pair + bias + argmax, stored as 16-byte vectors along w.
        // The two waves of a column half hold the two rows of the pooling pair in the accumulator layout (lane = column w,
        // registers = output channels).  Every tile goes through LDS once as a [32 co][32 w] fp32 image (4 KB, conflict
        // free both ways) and comes back transposed: lane = (co row, 4 consecutive w), so that a finished tile costs
        // 4 x 16-byte stores of pooled values + 4 x 4-byte stores of packed argmax bytes instead of 16 + 16 scalar ones
        // with their 64-bit address arithmetic (the scalar epilogue was ~1 300 instructions per wave and tile and a third
        // of the first block's time).  Two rounds, so that the 24 tiles in flight fit the LDS left by the K loop (96 KB):
        //   round 0: tiles 0,1,2 (finished by the row-0 wave) and 6,7,8 (row-1 wave);  round 1: tiles 3,4,5 and 9,10.
        float *xch = reinterpret_cast<float *>(smem);
        const int hp = h0 >> 1, Hp = a.H >> 1;
        const int co_l = lane >> 3, w4 = (lane & 7) * 4;                // transposed role of the lane inside a tile
        float bias_t[2][4];                                             // bias of the 4 co rows this lane stores, per channel half
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) bias_t[j][q] = a.bias[j * 32 + q * 8 + co_l];
        const bool want_stats = a.stats_part != nullptr;               // workgroup-uniform
        float slope_t[2][4];
        // The row sums are taken of t - shift_c with shift_c = PReLU(bias_c), the value of a plane whose convolution sum is
        // zero (silent clip, dead channel): sum and sum of squares in fp32 then carry no large common offset and
        // var = E[d^2] - E[d]^2 does not cancel for near-constant planes (mx_plane_stats_finish adds shift_c back).
        float shift_t[2][4];
        float st_s[2][4], st_q[2][4];                                   // [j = channel half ^ c][q]: sums over this lane's columns
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                slope_t[j][q] = want_stats ? a.slope_out[j * 32 + q * 8 + co_l] : 1.0f;
                shift_t[j][q] = bias_t[j][q] > 0.0f ? bias_t[j][q] : slope_t[j][q] * bias_t[j][q];
                st_s[j][q] = 0.0f;
                st_q[j][q] = 0.0f;
            }
        __syncthreads();                                                // the K loop's LDS images are dead
        constexpr int HALF = 3;                                         // tiles a wave finishes per exchange round: two rounds through 96 KB of LDS
        constexpr int ROUNDS = 6 / HALF, SLOTS = 2 * HALF;
#pragma unroll
        for (int round = 0; round < ROUNDS; ++round) {
            // slot s of a wave = tile i: s < HALF -> i = HALF round + s (row-0 finishes), s >= HALF -> i = 6 + HALF round + (s - HALF)
            float *mine = xch + (size_t)((c * 2 + row) * SLOTS) * 1024;
#pragma unroll
            for (int s6 = 0; s6 < SLOTS; ++s6) {
                const int i = s6 < HALF ? HALF * round + s6 : 6 + HALF * round + (s6 - HALF);
                if (i >= CV_WT) continue;
                store_tile32(acc, i, mine + s6 * 1024, lane);
            }
            __syncthreads();
            const float *top = xch + (size_t)((c * 2 + 0) * SLOTS) * 1024, *bot = xch + (size_t)((c * 2 + 1) * SLOTS) * 1024;
#pragma unroll
            for (int s3 = 0; s3 < HALF; ++s3) {
                const int s6 = row * HALF + s3;
                const int i = row == 0 ? HALF * round + s3 : 6 + HALF * round + s3;
                if (i >= CV_WT) continue;
                const int wt = i == 10 ? 5 : c * 6 + (i >> 1);           // column tile
                const int chh = i == 10 ? c : (i & 1) ^ c;              // channel half
                const int w = wt * 32 + w4;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = q * 8 + co_l;                       // co row inside the tile
                    const floatx4 tv = *reinterpret_cast<const floatx4 *>(top + s6 * 1024 + col * 32 + w4);
                    const floatx4 bv = *reinterpret_cast<const floatx4 *>(bot + s6 * 1024 + col * 32 + w4);
                    const float bsum = chh ? bias_t[1][q] : bias_t[0][q];
                    const float sl = chh ? slope_t[1][q] : slope_t[0][q];
                    const float sh = chh ? shift_t[1][q] : shift_t[0][q];
                    floatx4 m;
                    unsigned am = 0;
                    float ts = 0.0f, tq = 0.0f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool take_bot = bv[e] > tv[e];            // ties keep the first row (torch)
                        const float v = (take_bot ? bv[e] : tv[e]) * inv + bsum;
                        m[e] = w + e < a.Wv ? v : 0.0f;
                        am |= (take_bot ? 1u : 0u) << (8 * e);
                        const float t = m[e] > 0.0f ? m[e] : sl * m[e];
                        const float dlt = w + e < a.Wv ? t - sh : 0.0f;  // pad columns add nothing
                        ts += dlt;
                        tq += dlt * dlt;
                    }
                    // accumulator index j = channel half ^ c = i & 1 (tile 10: 0), the same for both rows' tiles of a slot:
                    // a compile-time constant after unrolling
                    st_s[(HALF * round + s3) & 1][q] += ts;
                    st_q[(HALF * round + s3) & 1][q] += tq;
                    const size_t off = (((size_t)b * CV_CO + chh * 32 + col) * Hp + hp) * CV_PITCH + w;
                    *reinterpret_cast<floatx4 *>(a.out + off) = m;
                    *reinterpret_cast<unsigned *>(a.out_amax + off) = am;
                }
            }
            if (round + 1 < ROUNDS) __syncthreads();                    // the next round overwrites the images
        }
        if (want_stats) {
            // [wave][j][q][lane] partial sums -> thread co < 64 adds the 4 waves x 8 column lanes of its channel in a fixed order
            __syncthreads();                                            // the round-1 images are dead
            const int wv = c * 2 + row;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    xch[((wv * 2 + j) * 4 + q) * 64 + lane] = st_s[j][q];
                    xch[2048 + ((wv * 2 + j) * 4 + q) * 64 + lane] = st_q[j][q];
                }
            __syncthreads();
            const int co = threadIdx.x;
            if (co < CV_CO) {
                const int chh = co >> 5, q = (co >> 3) & 3, col = co & 7;
                float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
                for (int w4i = 0; w4i < 4; ++w4i) {                     // wave (c, row): channel half chh sits in j = chh ^ c
                    const int j = chh ^ (w4i >> 1);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        s1 += xch[((w4i * 2 + j) * 4 + q) * 64 + col * 8 + e];
                        s2 += xch[2048 + ((w4i * 2 + j) * 4 + q) * 64 + col * 8 + e];
                    }
                }
                float *sp = a.stats_part + (((size_t)b * Hp + hp) * CV_CO + co) * 2;
                sp[0] = s1;
                sp[1] = s2;
            }
        }
    }
}

// Launched with OUTMODE 1 at T = 8 and 16 only (the dense data gradient); OUTMODE 0 is the forward it once ran, kept
// compilable: conv_f16x3_dma3_kernel below took it over and computes the same bits.
template <int T, int OUTMODE>      // OUTMODE 0: bias + maxpool + argmax, 1: plain rows
__global__ __launch_bounds__(256, 1) void conv_f16x3_kernel(ConvF16Args a)
{
    constexpr int PWP = CV_PITCH + 12 * T;            // patch positions per row (w = q - 6T)
    constexpr int WSL = CV_KW * 64 * 16;              // halfs per weight slab and split (13312)
    constexpr int PSL = 2 * PWP * 16;                 // halfs per patch and split (2 rows)
    constexpr int NWV = (2 * WSL / 8 + 255) / 256;    // 16-byte vectors per thread: weights (13)
    constexpr int NPI = 2 * 2 * PWP * 2;              // patch vectors: split x row x position x 2 halves
    constexpr int NPV = (NPI + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // LDS images keep the two 8-channel halves of a 16-channel block in separate planes, so that the 32 lanes of
    // a fragment read touch 32 CONSECUTIVE 16-byte chunks (conflict-free ds_read_b128; interleaving the halves
    // would put lanes l and l+8 on the same banks)
    _Float16 *wl = reinterpret_cast<_Float16 *>(smem);            // [split][kw][khalf][co][8]
    _Float16 *pl = wl + 2 * WSL;                                   // [split][row][khalf][q][8]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: wave-uniform address parts stay off the vector unit
    // wave = (output row, column half c).  Each wave owns all 64 output channels of 5 whole column tiles plus ONE
    // channel half of the middle tile (tile 5): 11 accumulators like a (channel half x whole row) split, but every
    // patch fragment feeds two channel tiles, so a tap needs 12 + 4 fragment reads instead of 22 + 2 -- the LDS
    // read pipe, shared by the four waves, was the co-limiter of the first version.
    //   acc[2t + j], t < 5 : column tile c*6 + t, channel half j ^ c;      acc[10] : column tile 5, channel half c
    const int row = wave >> 1, c = wave & 1, half = lane >> 5, l32 = lane & 31;
    // Workgroups go to the 8 XCDs round-robin in launch order: hand every XCD a CONTIGUOUS range of (clip, row pair)
    // tiles, so that the workgroups running together on one XCD are neighbouring row pairs of the same clips and
    // share their halo rows and weight stages in that XCD's L2 (speed only; any mapping is correct).
    int tile_id = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const int n_tiles = gridDim.x * gridDim.y;
        if ((n_tiles & 7) == 0) tile_id = (tile_id & 7) * (n_tiles >> 3) + (tile_id >> 3);
    }
    const int b = tile_id / gridDim.x, h0 = (tile_id - b * gridDim.x) * 2;

    floatx16 acc[CV_WT];
#pragma unroll
    for (int i = 0; i < CV_WT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    floatx4 wv[NWV], pv[NPV];
    // global loads of stage s = (cb, kh).  Branch-free: a predicated load is an exec-mask branch, and the 27 of them
    // with their address arithmetic sat between the two barriers of every stage; halo / out-of-image items read a
    // clamped (valid) address and are zeroed with a select.
    auto issue = [&](int s) {
        const int cb = s / CV_KH, kh = s - cb * CV_KH;
#pragma unroll
        for (int q = 0; q < NWV; ++q) {
            int i = tid + q * 256;
            const bool in = (2 * (WSL / 8)) % 256 == 0 || i < 2 * (WSL / 8);
            i = in ? i : 0;
            const int split = i / (WSL / 8), j = i - split * (WSL / 8);
            const _Float16 *src = (split ? a.w_lo : a.w_hi) + (size_t)(cb * CV_KH + kh) * WSL + (size_t)j * 8;
            wv[q] = *reinterpret_cast<const floatx4 *>(src);
        }
#pragma unroll
        for (int q = 0; q < NPV; ++q) {
            int i = tid + q * 256;
            const bool in = NPI % 256 == 0 || i < NPI;
            i = in ? i : 0;
            const int part = i & 1, pos = (i >> 1) % PWP, sr = (i >> 1) / PWP;     // sr = split * 2 + row
            const int split = sr >> 1, r = sr & 1;
            const int hx = h0 + r + kh - 2, w = pos - 6 * T;
            const bool ok = hx >= 0 && hx < a.H && w >= 0 && w < CV_PITCH;
            const int hx_c = hx < 0 ? 0 : (hx >= a.H ? a.H - 1 : hx), w_c = w < 0 ? 0 : (w >= CV_PITCH ? CV_PITCH - 1 : w);
            const _Float16 *src = (split ? a.x_lo : a.x_hi) + ((((size_t)b * a.H + hx_c) * 4 + cb) * CV_PITCH + w_c) * 16 + part * 8;
            const floatx4 v = *reinterpret_cast<const floatx4 *>(src);
            pv[q] = ok ? v : floatx4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto commit = [&]() {                                       // registers -> LDS
        floatx4 *wd = reinterpret_cast<floatx4 *>(wl);
#pragma unroll
        for (int q = 0; q < NWV; ++q) {
            const int i = tid + q * 256;
            if ((2 * (WSL / 8)) % 256 == 0 || i < 2 * (WSL / 8)) wd[i] = wv[q];             // the packed weights are the LDS image
        }
        floatx4 *pd = reinterpret_cast<floatx4 *>(pl);
#pragma unroll
        for (int q = 0; q < NPV; ++q) {
            const int i = tid + q * 256;
            if (NPI % 256 == 0 || i < NPI) {
                // item i = ((split*2 + row)*PWP + pos)*2 + part  ->  LDS [split][row][part][pos]
                const int part = i & 1, pos = (i >> 1) % PWP, sr = (i >> 1) / PWP;
                pd[(sr * 2 + part) * PWP + pos] = pv[q];
            }
        }
    };

    constexpr int N_STAGE = 4 * CV_KH;
    issue(0);
    for (int s = 0; s < N_STAGE; ++s) {
        __syncthreads();                                        // previous stage's fragments are all read
        commit();
        if (s + 1 < N_STAGE) issue(s + 1);                      // in flight during the MFMAs below
        __syncthreads();
        // fragment base addresses (halfs)
        const _Float16 *a0_hi_p = wl + (half * 64 + c * 32 + l32) * 8;                        // + kw * 1024
        const _Float16 *a1_hi_p = wl + (half * 64 + (c ^ 1) * 32 + l32) * 8;
        const _Float16 *b_hi_p = pl + ((size_t)(row * 2 + half) * PWP + c * 6 * 32 + l32) * 8;   // + (t*32 + kw*T) * 8
        const _Float16 *bm_hi_p = pl + ((size_t)(row * 2 + half) * PWP + 5 * 32 + l32) * 8;      // middle tile
        // two half-tap fragment sets: {tiles 0,1,2} and {tiles 3,4,middle}
        half8 a0h, a0l, a1h, a1l, n0h, n0l, n1h, n1l, bh0[3], bl0[3], bh1[3], bl1[3];
#define F16_LOAD_A(A0H, A0L, A1H, A1L, KW)                                        \
    A0H = *reinterpret_cast<const half8 *>(a0_hi_p + (KW) * (2 * 64 * 8));         \
    A0L = *reinterpret_cast<const half8 *>(a0_hi_p + WSL + (KW) * (2 * 64 * 8));   \
    A1H = *reinterpret_cast<const half8 *>(a1_hi_p + (KW) * (2 * 64 * 8));         \
    A1L = *reinterpret_cast<const half8 *>(a1_hi_p + WSL + (KW) * (2 * 64 * 8));
#define F16_LOAD_S0(KW)                                                                          \
    _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                              \
        bh0[i] = *reinterpret_cast<const half8 *>(b_hi_p + (i * 32 + (KW) * T) * 8);             \
        bl0[i] = *reinterpret_cast<const half8 *>(b_hi_p + PSL + (i * 32 + (KW) * T) * 8);       \
    }
#define F16_LOAD_S1(KW)                                                                          \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                              \
        bh1[i] = *reinterpret_cast<const half8 *>(b_hi_p + ((i + 3) * 32 + (KW) * T) * 8);       \
        bl1[i] = *reinterpret_cast<const half8 *>(b_hi_p + PSL + ((i + 3) * 32 + (KW) * T) * 8); \
    }                                                                                            \
    bh1[2] = *reinterpret_cast<const half8 *>(bm_hi_p + (KW) * T * 8);                           \
    bl1[2] = *reinterpret_cast<const half8 *>(bm_hi_p + PSL + (KW) * T * 8);
        F16_LOAD_A(a0h, a0l, a1h, a1l, 0)
        F16_LOAD_S0(0)
        F16_LOAD_S1(0)
#pragma unroll 1
        for (int kw = 0; kw < CV_KW; ++kw) {
            const int kn = kw + 1 < CV_KW ? kw + 1 : kw;         // last tap reloads itself (discarded)
            __builtin_amdgcn_sched_barrier(0);
            // the three split products of one accumulator are issued six MFMAs apart
#pragma unroll
            for (int i = 0; i < 3; ++i) { acc[2 * i] = mfma16(a0l, bh0[i], acc[2 * i]); acc[2 * i + 1] = mfma16(a1l, bh0[i], acc[2 * i + 1]); }
#pragma unroll
            for (int i = 0; i < 3; ++i) { acc[2 * i] = mfma16(a0h, bl0[i], acc[2 * i]); acc[2 * i + 1] = mfma16(a1h, bl0[i], acc[2 * i + 1]); }
#pragma unroll
            for (int i = 0; i < 3; ++i) { acc[2 * i] = mfma16(a0h, bh0[i], acc[2 * i]); acc[2 * i + 1] = mfma16(a1h, bh0[i], acc[2 * i + 1]); }
            __builtin_amdgcn_sched_barrier(0);
            F16_LOAD_A(n0h, n0l, n1h, n1l, kn)
            F16_LOAD_S0(kn)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 2; ++i) { acc[6 + 2 * i] = mfma16(a0l, bh1[i], acc[6 + 2 * i]); acc[7 + 2 * i] = mfma16(a1l, bh1[i], acc[7 + 2 * i]); }
            acc[10] = mfma16(a0l, bh1[2], acc[10]);
#pragma unroll
            for (int i = 0; i < 2; ++i) { acc[6 + 2 * i] = mfma16(a0h, bl1[i], acc[6 + 2 * i]); acc[7 + 2 * i] = mfma16(a1h, bl1[i], acc[7 + 2 * i]); }
            acc[10] = mfma16(a0h, bl1[2], acc[10]);
#pragma unroll
            for (int i = 0; i < 2; ++i) { acc[6 + 2 * i] = mfma16(a0h, bh1[i], acc[6 + 2 * i]); acc[7 + 2 * i] = mfma16(a1h, bh1[i], acc[7 + 2 * i]); }
            acc[10] = mfma16(a0h, bh1[2], acc[10]);
            __builtin_amdgcn_sched_barrier(0);
            F16_LOAD_S1(kn)
            a0h = n0h; a0l = n0l; a1h = n1h; a1l = n1l;
        }
#undef F16_LOAD_A
#undef F16_LOAD_S0
#undef F16_LOAD_S1
    }

    conv_f16_epilogue<OUTMODE>(acc, a, smem, b, h0, row, c, lane);
}

// ---- LDS-DMA version (T <= 4) ---------------------------------------------------------------------------
// Same tiling and arithmetic as conv_f16x3_kernel, but the operands travel global -> LDS by
// global_load_lds_dwordx4 (1 KiB per wave-instruction, no staging registers, no ds_write pass) into DOUBLE
// buffers, so that staging overlaps the MFMAs instead of sitting between two barriers:
//   LDS = W[2] (7 taps x 2 splits = 28 KB each) | P[2] (patch images [split][row][khalf][pos], 46-50 KB each)
// A stage (16 input channels x one kernel row) runs as two phases, taps 0..6 from W[0] and taps 7..12 from W[1]:
//   phase A issues  W[1] <- taps 7..12 of this stage,  first 8 pieces/wave of P[next] <- next stage's patch
//   phase B issues  W[0] <- taps 0..6 of the next stage, the remaining pieces of P[next]
// one DMA after every half tap (18 / 15 MFMAs), each phase ends with vmcnt(0) + barrier.  A DMA piece is 64
// consecutive 16-byte slots of the LDS image; every lane derives its own source address (halo / padding slots read
// a zero slot), precomputed once per kernel as a 32-bit descriptor per piece.
__device__ __attribute__((aligned(16))) unsigned k_zero_slot[4];

// One DMA piece: lane l's 16 bytes at gsrc land at LDS byte address lds_wave_base + 16 l.  Issued as inline asm on
// purpose: behind the __builtin the compiler books an LDS-DMA as a pending FLAT access and from then on turns every
// counted s_waitcnt lgkmcnt(n) of the fragment pipeline into lgkmcnt(0) (an MFMA bubble per tap); asm loads are
// invisible to its counters, so the waits for them are written by hand (DMA_WAIT before the phase barriers).
__device__ __forceinline__ void glds16(unsigned long long gsrc, unsigned lds_wave_base)
{
    unsigned keep;
    lds_wave_base = __builtin_amdgcn_readfirstlane(lds_wave_base);   // wave-uniform by construction; pin it to an SGPR
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_wave_base)
                 : "memory");
}
#define DMA_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

// Launched as the dense data gradient (plain rows * 1/S); the forward runs on conv_f16x3_dma16_kernel below.
template <int T>
__global__ __launch_bounds__(256, 1) void conv_f16x3_dma_kernel(ConvF16Args a)
{
    constexpr int NCB = 4, NKH = CV_KH;               // K stages: 4 channel blocks x 5 kernel rows
    constexpr int PWP = CV_PITCH + 12 * T;            // patch positions per row (w = q - 6T)
    constexpr int WSL = CV_KW * 64 * 16;              // halfs per packed weight stage and split
    constexpr int PLANE = PWP * 16;                   // bytes of one (split, row, khalf) plane
    constexpr int P_SLOTS = 8 * PWP;
    constexpr int P_PIECES = (P_SLOTS + 63) / 64;
    constexpr int P_BYTES = P_PIECES * 1024;
    constexpr int PPW = (P_PIECES + 3) / 4;           // patch pieces per wave (12..13)
    constexpr int W_SPLIT = 7 * 2048;                 // bytes per split inside a weight buffer
    constexpr int W_BYTES = 2 * W_SPLIT;
    constexpr int ROWB = NCB * CV_PITCH * 32;         // bytes of one operand row (channel blocks x 352 positions x 16 halfs)
    constexpr int N_STAGE = NCB * NKH;
    static_assert(PPW <= 13, "patch pieces per wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *const W0 = smem, *const W1 = smem + W_BYTES, *const P0 = smem + 2 * W_BYTES;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;   // LDS byte address

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = wave >> 1, c = wave & 1, half = lane >> 5, l32 = lane & 31;
    // Workgroups go to the 8 XCDs round-robin in launch order: hand every XCD a CONTIGUOUS range of (clip, row pair)
    // tiles, so that the workgroups running together on one XCD are neighbouring row pairs of the same clips and
    // share their halo rows and weight stages in that XCD's L2 (speed only; any mapping is correct).
    int tile_id = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const int n_tiles = gridDim.x * gridDim.y;
        if ((n_tiles & 7) == 0) tile_id = (tile_id & 7) * (n_tiles >> 3) + (tile_id >> 3);
    }
    const int b = tile_id / gridDim.x, h0 = (tile_id - b * gridDim.x) * 2;

    floatx16 acc[CV_WT];
#pragma unroll
    for (int i = 0; i < CV_WT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    // patch piece descriptors: bit 31 = no source (halo column / padding slot), bit 30 = split, bit 29 = row,
    // low bits = byte offset of the slot's 16 bytes from the stage's first row
    int desc[PPW];
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int i = (wave + 4 * k) * 64 + lane;
        const int plane = i / PWP, pos = i - plane * PWP, w = pos - 6 * T;
        const int split = plane >> 2, r = (plane >> 1) & 1, part = plane & 1;
        desc[k] = (i < P_SLOTS && w >= 0 && w < CV_PITCH) ? ((split << 30) | (r << 29) | (r * ROWB + w * 32 + part * 16)) : -1;
    }
    // plain integer addresses (selecting between kernel-argument FIELDS per lane would make the compiler load the
    // pointer through memory and wait for it -- and with it for every DMA in flight)
    const unsigned long long zero_src = (unsigned long long)k_zero_slot, xh = (unsigned long long)a.x_hi,
                             xl = (unsigned long long)a.x_lo, wh = (unsigned long long)a.w_hi, wlo = (unsigned long long)a.w_lo;
    const int H = a.H;

    // A DMA slot = (lane source address, wave LDS base).  The address arithmetic is separated from the issue and every
    // slot is issued UNCONDITIONALLY: a slot without a piece (no next stage; a wave's last, out-of-range piece) repeats
    // a harmless one -- the current stage's data into the buffer nobody reads any more, or the wave's previous piece
    // once more.  Without conditions the ~15 VALU / SALU instructions of the address are straight-line code in front
    // of the slot and execute in the shadow of the MFMAs there; behind a branch they were sunk into the slot's own
    // basic block, a matrix-pipe bubble twice per tap.
    struct DmaSlot { unsigned long long src; unsigned lds; };
    // weights of (stage, taps [t0, t0 + nt)) -> Wb; piece pw of the 2 * nt * 2 covers one (split, tap, khalf) plane
    auto slot_w = [&](int st, int t0, int nt, unsigned char *Wb, int j) {
        const int pw = wave + 4 * j, per = 2 * nt;
        const int split = pw / per, rem = pw - split * per;
        DmaSlot d;
        d.src = (split ? wlo : wh) + ((unsigned long long)st * WSL + (t0 * 2 + rem) * 512 + lane * 8) * 2;
        d.lds = lds0 + (unsigned)(Wb - smem) + split * W_SPLIT + rem * 1024;
        return d;
    };
    // patch piece k of stage st -> Pb (k >= 1 when the wave's piece k can be out of range: then piece k - 1 again)
    auto slot_p = [&](int st, unsigned char *Pb, int k) {
        const bool in_range = wave + 4 * k < P_PIECES;
        const int pp = in_range ? wave + 4 * k : wave + 4 * (k - 1);
        const int d = in_range ? desc[k] : desc[k > 0 ? k - 1 : 0];
        const int cb = st / NKH, kh = st - cb * NKH, hx0 = h0 + kh - NKH / 2;
        const bool v0 = hx0 >= 0 && hx0 < H, v1 = hx0 + 1 >= 0 && hx0 + 1 < H;
        const long long st_off = (((long long)b * H + hx0) * NCB + cb) * (CV_PITCH * 32);
        const unsigned long long base_h = xh + st_off, base_l = xl + st_off;
        const bool ok = d >= 0 && ((d & (1 << 29)) ? v1 : v0);
        const unsigned long long src = ((d & (1 << 30)) ? base_l : base_h) + (unsigned)(d & 0xFFFFF);
        DmaSlot r;
        r.src = ok ? src : zero_src;
        r.lds = lds0 + (unsigned)(Pb - smem) + pp * 1024;
        return r;
    };
    auto slot_issue = [&](const DmaSlot &d) { glds16(d.src, d.lds); };
    auto dma_w = [&](int st, int t0, int nt, unsigned char *Wb, int j) { slot_issue(slot_w(st, t0, nt, Wb, j)); };
    auto dma_p = [&](int st, unsigned char *Pb, int k) { if (wave + 4 * k < P_PIECES) slot_issue(slot_p(st, Pb, k)); };

    // prologue: taps 0..6 of stage 0 and its patch
#pragma unroll
    for (int j = 0; j < 7; ++j) dma_w(0, 0, 7, W0, j);
#pragma unroll
    for (int k = 0; k < PPW; ++k) dma_p(0, P0, k);
    DMA_WAIT();
    __syncthreads();

#pragma unroll 1
    for (int s = 0; s < N_STAGE; ++s) {
        unsigned char *const Pc = P0 + (s & 1) * P_BYTES, *const Pn = P0 + ((s + 1) & 1) * P_BYTES;
        const bool more = s + 1 < N_STAGE;
        const int sn = more ? s + 1 : s;             // the stage whose operands the DMA slots fetch (see DmaSlot)
        const unsigned char *b_p = Pc + (row * 2 + half) * PLANE + (c * 6 * 32 + l32) * 16;      // + split*4*PLANE + (t*32 + kw*T)*16
        const unsigned char *bm_p = Pc + (row * 2 + half) * PLANE + (5 * 32 + l32) * 16;         // middle tile
        // fragments of one tap, double buffered (FA: a0h a0l a1h a1l; FBH/FBL: tiles 0..4 + the middle tile)
        half8 FA[2][4], FBH[2][6], FBL[2][6];
        // read r (0..15) of the tap (weights buffer Wb, local tap tl, kernel column kw) into fragment set f
        auto rd = [&](int f, const unsigned char *Wb, int tl, int kw, int r) {
            if (r < 4) {
                const int ch = (r >> 1) ? (c ^ 1) : c;
                FA[f][r] = *reinterpret_cast<const half8 *>(Wb + (r & 1) * W_SPLIT + (tl * 2 + half) * 1024 + (ch * 32 + l32) * 16);
            } else {
                const int tile = (r - 4) >> 1, lo = (r - 4) & 1;
                const unsigned char *p = (tile < 5 ? b_p + tile * 32 * 16 : bm_p) + lo * 4 * PLANE + kw * T * 16;
                if (lo) FBL[f][tile] = *reinterpret_cast<const half8 *>(p);
                else FBH[f][tile] = *reinterpret_cast<const half8 *>(p);
            }
        };
        // MFMA i (0..32) of the tap: term (lo*hi, hi*lo, hi*hi) x 11 accumulators, so that one accumulator is touched
        // every 11th instruction
        auto mma = [&](int f, int i) {
            const int term = i / 11, u = i - term * 11;
            const int tile = u < 10 ? (u >> 1) : 5, j = u < 10 ? (u & 1) : 0;
            const half8 av = FA[f][2 * j + (term == 0 ? 1 : 0)];
            const half8 bv = term == 1 ? FBL[f][tile] : FBH[f][tile];
            acc[u] = mfma16(av, bv, acc[u]);
        };
        // One tap: 33 MFMAs on set f, the next tap's 16 fragment reads into set f^1 (r_lo..15; r_lo = 4 skips the
        // weights, 16 skips everything), one read after every second MFMA, and two DMA slots.  The wave issues in
        // order, so anything clustered between MFMA groups is a matrix-pipe bubble: the interleave is pinned.
#define DMA_TAP(F, WB, TLN, KWN, R_LO, NA, SLOT_A, SLOT_A2, NB, SLOT_B, SLOT_B2)                  \
    {                                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        const DmaSlot sa_ = SLOT_A, sa2_ = SLOT_A2;                                              \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) mma(F, i);                                \
        _Pragma("unroll") for (int r = 0; r < 8; ++r) if (r >= (R_LO)) rd((F) ^ 1, WB, TLN, KWN, r); \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                          \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                   \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                   \
        }                                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if ((NA) >= 1) slot_issue(sa_);                                                          \
        if ((NA) >= 2) slot_issue(sa2_);                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        const DmaSlot sb_ = SLOT_B, sb2_ = SLOT_B2;                                              \
        _Pragma("unroll") for (int i = 16; i < 33; ++i) mma(F, i);                               \
        _Pragma("unroll") for (int r = 8; r < 16; ++r) if (r >= (R_LO)) rd((F) ^ 1, WB, TLN, KWN, r); \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                          \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                   \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                   \
        }                                                                                        \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                       \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if ((NB) >= 1) slot_issue(sb_);                                                          \
        if ((NB) >= 2) slot_issue(sb2_);                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
    }
        // DMA schedule.  The end of a phase waits for the pieces its successor reads, so nothing it needs is issued
        // late: a piece requested in the last slot cost a full memory round trip at the barrier, twice per stage.
        //   phase A (14 slots): W1 <- this stage's taps 7..12 in slots 0..5, then patch pieces 0..7 of the next stage;
        //           its end waits with vmcnt(8): the six weight pieces, not the eight patch pieces behind them
        //   phase B (12 slots): W0 <- the next stage's taps 0..6 in slots 0..6 and the remaining patch pieces 8.. riding
        //           along in slots 0.. (two pieces per slot); the last five slots are empty
        static_assert(PPW >= 12 && PPW <= 15, "DMA schedule");
#define DMA_SLOT_A(J) ((J) < 6 ? slot_w(s, 7, 6, W1, (J)) : slot_p(sn, Pn, (J) - 6))
#define DMA_NB(J) (((J) < 7 ? 1 : 0) + ((J) + 8 < PPW ? 1 : 0))
#define DMA_SLOT_B(J) slot_w(sn, 0, 7, W0, (J) < 7 ? (J) : 0)
#define DMA_SLOT_B2(J) slot_p(sn, Pn, (J) + 8 < PPW ? (J) + 8 : PPW - 1)

        // ---- phase A: taps 0..6 from W0
#pragma unroll
        for (int r = 0; r < 16; ++r) rd(0, W0, 0, 0, r);
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            if (t < 6) DMA_TAP(t & 1, W0, t + 1, t + 1, 0, 1, DMA_SLOT_A(2 * t), DMA_SLOT_A(2 * t), 1, DMA_SLOT_A(2 * t + 1), DMA_SLOT_A(2 * t + 1))
            else DMA_TAP(t & 1, W0, 0, 7, 4, 1, DMA_SLOT_A(2 * t), DMA_SLOT_A(2 * t), 1, DMA_SLOT_A(2 * t + 1), DMA_SLOT_A(2 * t + 1))     // tap 7's patch fragments only
        }
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");     // this wave's W1 pieces landed (8 patch pieces may be in flight) ...
        __syncthreads();                       // ... and everyone's did
        // ---- phase B: taps 7..12 from W1 (fragment set 1 holds tap 7's patch fragments)
#pragma unroll
        for (int r = 0; r < 4; ++r) rd(1, W1, 0, 7, r);
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            if (t < 5) DMA_TAP((t + 1) & 1, W1, t + 1, 8 + t, 0, DMA_NB(2 * t), DMA_SLOT_B(2 * t), DMA_SLOT_B2(2 * t), DMA_NB(2 * t + 1), DMA_SLOT_B(2 * t + 1), DMA_SLOT_B2(2 * t + 1))
            else DMA_TAP((t + 1) & 1, W1, 0, 0, 16, DMA_NB(2 * t), DMA_SLOT_B(2 * t), DMA_SLOT_B2(2 * t), DMA_NB(2 * t + 1), DMA_SLOT_B(2 * t + 1), DMA_SLOT_B2(2 * t + 1))
        }
        DMA_WAIT();
        __syncthreads();
#undef DMA_TAP
#undef DMA_SLOT_A
#undef DMA_SLOT_B
#undef DMA_SLOT_B2
#undef DMA_NB
    }
    conv_f16_epilogue<1>(acc, a, smem, b, h0, row, c, lane);
}

// ---- first block, persistent, TILE-OUTER (2 input channels as a k-vector operand: ONE K stage of 13 taps per output row pair) ----
// A workgroup walks a contiguous range of row pairs; the next row pair's patch arrives by LDS-DMA during the current one's taps.
// The row-pair-outer kernels this one replaced (retired) kept all 176 accumulator registers of a row pair alive
// through its 13 taps and then ran a 14 k-cycle epilogue that nothing overlapped: one wave per SIMD, taps and epilogue simply
// add (15.0 k + 14.4 k cycles per row pair).  The
// first block is special: K = 13 taps x 16 "channels" only, so the WEIGHTS of a wave's 32 output channels fit in registers
// (13 taps x {hi, lo} x 4 = 104) and the loops can be turned inside out:
//   for each 32-column tile:  both rows of the pooling pair x 13 taps x 3 split products = 78 matrix instructions on TWO
//   accumulators (32 registers), patch fragments straight from the LDS image (4 ds_read_b128 per tap, one tap ahead),
// and the tile is DONE: its max-pool, transposition through the wave's private LDS image, bias, LayerNorm partial sums and
// 16-byte stores run, cut into pieces, in the shadow of the matrix instructions of tile t + 1
// (two accumulator sets, ping-pong), with no workgroup barrier inside a row pair.
// Waves = (channel tile jt, column half c); 352 columns = 11 tiles: c = 0 takes tiles 0..5, c = 1 tiles 5..10 -- tile 5 is
// computed by both (bit-identical values, stored twice; its partial sums are counted once): 6 x 78 = 468 instead of 429 matrix
// instructions per wave and row pair, in exchange for no cross-wave exchange of the middle tile.
// (A first version with swapped operands -- a lane = one channel, 16-byte stores straight from the accumulators, no LDS at all
//  -- was store-bound: 64 scattered 16-byte pieces per store instruction, 2.1 ms for the stores alone.)
//   LDS = P[2] (46 KB each: the row pair's patch, LDS-DMA double buffered) | 4 transposition images (17 KB) | sums (8 KB) | DMA descriptors (12 KB)
// Measured (one box, 256 clips x 256 mel bins): 2.23 -> 2.06 ms inside the train step, 1.97 -> 1.92 ms alone.  Ablations (alone):
// without the matrix instructions 1.18 ms, without the global stores 1.68 ms: ~2 500 vector / LDS / store instructions ride on 468
// matrix instructions per row pair, and a lone wave issues one of them per ~7 cycles -- the wave is VECTOR-ISSUE bound (17.6 k
// cycles of issue against 15 k of matrix pipe), the two now overlap only where the interleave is even (the scheduler still
// leaves ~30 of the 468 gaps with 17-37 instructions).  Tried and dropped: the tile stream continued ACROSS row pairs (the last
// tile's epilogue under the next pair's first tile, sums exchanged one pair late): parity-green, 2.27 ms in the step -- the
// accumulators carried around the loop cost 100 more AGPR copies than the exposed epilogue saved.
#ifndef C1T_ABL
#define C1T_ABL 0       // ablation knobs of the tile-outer kernel (wrong results; tools/exp_block1.py): 1 no epilogue, 2 no matrix instructions, 4 no global stores, 8 no LDS-DMA in the loop
#endif
struct Conv1Consts { float bias[4], slope[4], nshift[4]; };          // of channel rows jt*32 + q*8 + (lane >> 3): loaded once per workgroup
__device__ __forceinline__ Conv1Consts conv1_consts(const ConvF16Args &a, int jt, int lane)
{
    Conv1Consts k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        k.bias[q] = a.bias[jt * 32 + q * 8 + (lane >> 3)];
        k.slope[q] = a.stats_part != nullptr ? a.slope_out[jt * 32 + q * 8 + (lane >> 3)] : 1.0f;
        k.nshift[q] = -(k.bias[q] > 0.0f ? k.bias[q] : k.slope[q] * k.bias[q]);
    }
    return k;
}
template <bool STATS>     // STATS: leave the next block's LayerNorm partial sums (stats_part / slope_out given); a template so that a tile's epilogue is branch-free
__global__ __launch_bounds__(256, 1) void conv1_f16x3_tile_kernel(ConvF16Args a, int n_tiles, int tiles_per_wg)
{
    constexpr int T = 1;
    constexpr int PWP = CV_PITCH + 12 * T;
    constexpr int PLANE = PWP * 16;
    constexpr int P_SLOTS = 8 * PWP;
    constexpr int P_PIECES = (P_SLOTS + 63) / 64;
    constexpr int P_BYTES = P_PIECES * 1024;
    constexpr int PPW = (P_PIECES + 3) / 4;                      // 12
    constexpr int ROWB = CV_PITCH * 32;
    constexpr int NT = 6;                                        // column tiles per wave
    static_assert(PPW == 12, "DMA schedule");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *const P0 = smem;
    unsigned char *const scr = smem + 2 * P_BYTES;                           // 4 waves x 4352 B: [32 co][32 w] image + 64 flag words
    float *const xch = reinterpret_cast<float *>(scr + 4 * 4352);            // [2][wave * 4 + q][64 lanes]
    int *const desc_l = reinterpret_cast<int *>(scr + 4 * 4352 + 8192);      // [piece k][thread]: the DMA descriptors (12 registers otherwise)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jt = wave >> 1, c = wave & 1, half = lane >> 5, l32 = lane & 31;
    int wg = blockIdx.x;
    if ((gridDim.x & 7) == 0) wg = (wg & 7) * (gridDim.x >> 3) + (wg >> 3);
    const int t_begin = wg * tiles_per_wg, t_end = min(t_begin + tiles_per_wg, n_tiles);
    if (t_begin >= t_end) return;
    const int Hp = a.H >> 1, H = a.H;
    auto make_desc = [&](int k) {
        const int i = (wave + 4 * k) * 64 + lane;
        const int plane = i / PWP, pos = i - plane * PWP, w = pos - 6 * T;
        const int split = plane >> 2, r = (plane >> 1) & 1, part = plane & 1;
        return (i < P_SLOTS && w >= 0 && w < CV_PITCH) ? ((split << 30) | (r << 29) | (r * ROWB + w * 32 + part * 16)) : -1;
    };
    const unsigned long long zero_src = (unsigned long long)k_zero_slot, xh = (unsigned long long)a.x_hi, xl = (unsigned long long)a.x_lo;
    // patch piece k (descriptor d) of row pair `tile` -> patch buffer pb; a wave without a piece k repeats its piece k - 1 (harmless)
    auto issue_piece = [&](int tile, int pb, int k, int d) {
        const int pp = wave + 4 * k < P_PIECES ? wave + 4 * k : wave + 4 * (k - 1);
        const int tb = tile / Hp, th0 = (tile - tb * Hp) * 2;
        const long long st_off = ((long long)tb * H + th0) * (CV_PITCH * 32);
        const unsigned long long src = ((d & (1 << 30)) ? xl : xh) + st_off + (unsigned)(d & 0xFFFFF);
        glds16(d >= 0 ? src : zero_src, lds0 + pb * P_BYTES + pp * 1024);
    };
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int d = make_desc(wave + 4 * k < P_PIECES ? k : k - 1);
        desc_l[k * 256 + tid] = d;
        if (wave + 4 * k < P_PIECES) issue_piece(t_begin, 0, k, d);
    }

    // the wave's weights: A operand, lane (row = channel jt*32 + l32, k half) -> 8 halfs of [kw][khalf][co][8]
    half8 WH[CV_KW], WL[CV_KW];
#pragma unroll
    for (int kw = 0; kw < CV_KW; ++kw) {
        const size_t o = ((size_t)(kw * 2 + half) * 64 + jt * 32 + l32) * 8;
        WH[kw] = *reinterpret_cast<const half8 *>(a.w_hi + o);
        WL[kw] = *reinterpret_cast<const half8 *>(a.w_lo + o);
    }
    // the loads have landed BEFORE the loop as far as the compiler is concerned too: otherwise its wait-count pass guards the first
    // tile's matrix instructions of EVERY row pair with vmcnt(24) .. vmcnt(0) -- which in the steady state waits for the previous
    // row pair's stores to retire (first version of this kernel: 2.7 ms)
#pragma unroll
    for (int kw = 0; kw < CV_KW; ++kw) asm volatile("" : "+v"(WH[kw]), "+v"(WL[kw]));
    // transposed role of the lane in the epilogue (a finished tile comes back from the wave's LDS image as [co][w]): 4 channel
    // rows q*8 + co_l, 4 columns w4 .. w4 + 3
    const Conv1Consts kc = conv1_consts(a, jt, lane);
    const int co_l = lane >> 3, w4 = (lane & 7) * 4, rbit0 = co_l & 3, fhalf = (co_l >> 2) & 1;
    float *const img = reinterpret_cast<float *>(scr + wave * 4352);
    unsigned *const flg = reinterpret_cast<unsigned *>(scr + wave * 4352 + 4096);
    unsigned voff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) voff[q] = (unsigned)((q * 8 + co_l) * Hp * CV_PITCH + w4);
    const float inv = 1.0f / F16_WSCALE;
    const int tile0 = c ? 5 : 0;                                  // first column tile of this wave
    const float tile5_w = c ? 0.0f : 1.0f;                        // column tile 5 is computed by both column-half waves: its sums count once
    DMA_WAIT();
    __syncthreads();

#pragma unroll 1
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int pb = (tile - t_begin) & 1;
        const unsigned char *const Pc = P0 + pb * P_BYTES;
        const int tn = tile + 1 < t_end ? tile + 1 : tile;
        const int b = tile / Hp, hp = tile - b * Hp;
        const size_t sbase = (((size_t)b * CV_CO + jt * 32) * Hp + hp) * CV_PITCH;      // wave-uniform
        float *const out_b = a.out + sbase;
        unsigned char *const amax_b = a.out_amax + sbase;
        // patch fragment (B operand): lane (column = position l32, k half) of plane (split, row r, k half) at column tile*32 + l32 + kw
        const unsigned char *const fr = Pc + half * PLANE + (tile0 * 32 + l32) * 16;
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        floatx16 acc[2][2];                                       // [set][row]
        half8 F[2][4];                                            // [buffer][row * 2 + split]
        auto rd = [&](int buf, int t, int kw) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                F[buf][q] = *reinterpret_cast<const half8 *>(fr + ((q & 1) * 4 + (q >> 1) * 2) * PLANE + t * 512 + kw * 16);
        };
        // ---- the epilogue of a finished tile, in pieces.  A: max over the pair + flags -> the wave's image ([co][w], in the
        // accumulator layout: lane = column, register = channel row); B: read back transposed (lane = 4 channel rows x 4 columns);
        // C(q): bias, LayerNorm partial sums, 16-byte store of channel row q*8 + co_l
        uint4 flw;
        floatx4 tvq[4], mq;
        unsigned flags = 0;
        auto epi_a = [&](int set, int r0) {                       // four channel rows per call (taps 0..3)
            if (r0 == 0) flags = 0;
#pragma unroll
            for (int r = r0; r < r0 + 4; ++r) {
                const bool take_bot = acc[set][1][r] > acc[set][0][r];         // ties keep the first row (torch)
                img[mfma_row(r, lane) * 32 + l32] = take_bot ? acc[set][1][r] : acc[set][0][r];
                flags |= (take_bot ? 1u : 0u) << r;
            }
            if (r0 == 12) flg[lane] = flags;
        };
        auto epi_b = [&]() {                                      // (the wave's own LDS operations execute in order: no barrier)
            flw = *reinterpret_cast<const uint4 *>(flg + fhalf * 32 + w4);
#pragma unroll
            for (int q = 0; q < 4; ++q) tvq[q] = *reinterpret_cast<const floatx4 *>(img + (q * 8 + co_l) * 32 + w4);
        };
        auto epi_c1 = [&](int t, int q) {                         // bias, pad mask, argmax bytes, the two stores
            const int wt = tile0 + t, w = wt * 32 + w4;
            const unsigned fl[4] = {flw.x, flw.y, flw.z, flw.w};
            const floatx4 invv = {inv, inv, inv, inv}, bv4 = {kc.bias[q], kc.bias[q], kc.bias[q], kc.bias[q]};
            floatx4 m = __builtin_elementwise_fma(tvq[q], invv, bv4);
            unsigned am = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) am |= ((fl[e] >> (q * 4 + rbit0)) & 1u) << (8 * e);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = w + e < a.Wv ? m[e] : 0.0f;
            mq = m;
            if ((C1T_ABL & 4) && m[0] + m[1] + m[2] + m[3] != 12345.0f && am != 77u) return;       // ablation: no global stores
            *reinterpret_cast<floatx4 *>(out_b + (voff[q] + (unsigned)(wt * 32))) = m;
            *reinterpret_cast<unsigned *>(amax_b + (voff[q] + (unsigned)(wt * 32))) = am;
        };
        auto epi_c2 = [&](int t, int q) {                         // LayerNorm partial sums of PReLU(out) - PReLU(bias)
            if (!STATS) return;
            const int w = (tile0 + t) * 32 + w4;
            const floatx4 m = mq;
            const floatx4 sm = m * floatx4{kc.slope[q], kc.slope[q], kc.slope[q], kc.slope[q]};
            floatx4 d;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = (m[e] > 0.0f ? m[e] : sm[e]) + kc.nshift[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = w + e < a.Wv ? d[e] : 0.0f;                // pad columns add nothing
            if (t == 0) d = d * floatx4{tile5_w, tile5_w, tile5_w, tile5_w};             // (t == 0 of the c = 1 wave is column tile 5 again)
            s1[q] += (d[0] + d[1]) + (d[2] + d[3]);
            const floatx4 dd = d * d;
            s2[q] += (dd[0] + dd[1]) + (dd[2] + dd[3]);
        };
        rd(0, 0, 0);
        int dnext = -1;
#pragma unroll
        for (int t = 0; t <= NT; ++t) {
            const int set = t & 1;
            if (t < NT) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[set][r][i] = 0.0f;
            }
#pragma unroll
            for (int kw = 0; kw < CV_KW; ++kw) {
                const int f = (t * CV_KW + kw) & 1;
                __builtin_amdgcn_sched_barrier(0);
                if (t < NT && (C1T_ABL & 2)) {
                    acc[set][0][kw] += (float)F[f][0][0] + (float)F[f][1][1] + (float)WL[kw][0];      // keep the reads alive
                    acc[set][1][kw] += (float)F[f][2][0] + (float)F[f][3][1] + (float)WH[kw][0];
                    if (kw + 1 < CV_KW) rd(f ^ 1, t, kw + 1);
                    else if (t + 1 < NT) rd(f ^ 1, t + 1, 0);
                }
                if (t < NT && !(C1T_ABL & 2)) {
                    // split products in the order of the other kernels: w_lo x p_hi, w_hi x p_lo, w_hi x p_hi
                    acc[set][0] = mfma16(WL[kw], F[f][0], acc[set][0]);
                    acc[set][1] = mfma16(WL[kw], F[f][2], acc[set][1]);
                    acc[set][0] = mfma16(WH[kw], F[f][1], acc[set][0]);
                    acc[set][1] = mfma16(WH[kw], F[f][3], acc[set][1]);
                    acc[set][0] = mfma16(WH[kw], F[f][0], acc[set][0]);
                    acc[set][1] = mfma16(WH[kw], F[f][2], acc[set][1]);
                    if (kw + 1 < CV_KW) rd(f ^ 1, t, kw + 1);
                    else if (t + 1 < NT) rd(f ^ 1, t + 1, 0);
                }
                // the previous tile's epilogue in the matrix instructions' shadow: A over taps 0..1, B at tap 3, C(q) at taps 5, 7, 9, 11
                if (t > 0 && !(C1T_ABL & 1)) {
                    if (kw < 4) epi_a(set ^ 1, 4 * kw);
                    if (kw == 4) epi_b();
                    if (kw >= 5 && (kw & 1)) epi_c1(t - 1, (kw - 5) >> 1);         // taps 5, 7, 9, 11
                    if (kw >= 6 && !(kw & 1)) epi_c2(t - 1, (kw - 6) >> 1);        // taps 6, 8, 10, 12
                }
                // two DMA pieces of the next row pair's patch per tile (descriptor read from LDS a tap earlier)
                if (t < NT && (kw == 3 || kw == 8)) dnext = desc_l[(2 * t + (kw == 8 ? 1 : 0)) * 256 + tid];
                if (t < NT && (kw == 4 || kw == 9) && !(C1T_ABL & 8)) issue_piece(tn, pb ^ 1, 2 * t + (kw == 9 ? 1 : 0), dnext);
                if (t < NT) {
#pragma unroll
                    for (int q_ = 0; q_ < 6; ++q_) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
                        __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);      // VALU
                        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);      // DS write
                        __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);      // VMEM write
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the next patch has landed: its last piece was issued at (tile 5, tap 9); behind it in program order sit the 2 + 8 stores of
        // the last epilogue pieces, which need not have retired (vmcnt retires in order: <= 10 outstanding = every DMA piece is in)
        asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        if (STATS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                xch[(wave * 4 + q) * 64 + lane] = s1[q];
                xch[1024 + (wave * 4 + q) * 64 + lane] = s2[q];
            }
        }
        __syncthreads();                                          // patch buffer pb is free; the other one is visible; sums exchanged
        if (STATS) {
            // [wave][q][lane] partial sums -> thread co < 64 adds the 2 waves x 8 column lanes of its channel in a fixed order
            const int co = threadIdx.x;
            if (co < CV_CO) {
                const int cjt = co >> 5, q = (co >> 3) & 3, col = co & 7;
                float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
                for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        t1 += xch[((cjt * 2 + cc) * 4 + q) * 64 + col * 8 + e];
                        t2 += xch[1024 + ((cjt * 2 + cc) * 4 + q) * 64 + col * 8 + e];
                    }
                float *sp = a.stats_part + (((size_t)b * Hp + hp) * CV_CO + co) * 2;
                sp[0] = t1;
                sp[1] = t2;
            }
            __syncthreads();                                      // (the exchange slots are rewritten by the next row pair)
        }
    }
}

// ---- LDS-DMA version on v_mfma_f32_16x16x32_f16 (forward, T <= 4) -------------------------------------------------
// Same workgroup tile, wave tile (64 channels x 5.5 column tiles = 176 accumulator registers), operand images, LDS-DMA
// staging and epilogue as conv_f16x3_dma_kernel; only the matrix instruction differs.  Why: these kernels are power
// limited (matrix pipes ~84 % busy at 1.6-1.7 GHz), and at equal cycles per FLOP the chip holds a higher clock on the
// 16x16x32 shape than on 32x32x16 -- tools/probe/ubench_mfma_shape.hip at this wave tile, random fp16 operands re-read
// from LDS: 1 880 against 1 653 TFLOP/s (1.87 against 1.65 GHz, loop cycles equal within 0.2 %).
//   K = 32 of one instruction = a PAIR of taps x 16 input channels: lane group g = lane >> 4 holds (tap parity g >> 1,
//   8-channel half g & 1), so both operands are still ONE ds_read_b128 per fragment out of the unchanged images
//   (weights [split][tap][khalf][co][8], patch [split][row][khalf][pos][8]); a 32 x 32 output tile is 2 x 2
//   accumulators and its four instructions share two A and two B fragments: the same LDS bytes per FLOP.
//   13 taps per stage is odd.  Padding tap 12 with a zero tap (first version: 14 / 13 of the matrix work) ate the gain:
//   isolated 12.9 -> 12.2 ms, inside the train step 12.64 -> 12.84 ms.  So stages run in (even, odd) couples of 26 taps =
//   13 pairs: the even stage runs taps 0..11 and leaves tap 12; the odd stage starts with the STRADDLING pair (tap 12
//   of the even stage, tap 0 of the odd one) -- at that moment both stages' weights and patches are resident (the
//   double buffers) -- then taps 1..12.  The straddling pair's lanes address two different buffers (per-lane bases).
//   Its operands must be read before the odd stage's DMA overwrites the even stage's patch: W1's tap-12 slot is never
//   written in an odd stage, the patch pieces are issued only after a workgroup barrier behind the straddling pair.
//   Buffers (7 tap slots each):   even stage: W0 = taps 0..5, W1 = taps 6..12;   odd stage: W0 = taps 0..6, W1 = taps 7..12.
//   Instruction order inside a pair: column tile by column tile (12 instructions = 3 terms x 4 channel tiles, one
//   accumulator every 4th instruction); a tile's two B fragments are dead after its 12 instructions, so the patch
//   fragments live in a RING of six tiles read four tiles ahead of their use (across pair boundaries), and only the 8 A
//   fragments are double buffered: 12 + 16 fragment vectors (112 registers).
#ifndef DMA16_ABL
#define DMA16_ABL 0     // ablation knob (wrong results): 2 = no barrier behind the straddling pair
#endif
// The patch lives in a ring of FOUR ROW SLOTS (the first version: two 2-row buffers, P0 / P1 in the notes above).  Stage (cb, kh) reads input rows
//   j = kh (for output row 0) and kh + 1 (output row 1) of the six rows j = 0..5 = h0 - 2 .. h0 + 3 of channel block cb;
//   row number n = 6 cb + j lives in slot n & 3.  Consecutive kernel-row stages of a channel block share a row, so a stage
//   fetches ONE new row for its successor (its row kh + 1), and a second one (row 0, in one burst behind the mid-stage
//   barrier) only when the successor opens a channel block: 6 instead of 10 row fetches per channel block = 40 % fewer
//   patch pieces, 19 % fewer LDS-DMA pieces in all (each one costs issue slots between 16-cycle matrix instructions and
//   energy: the kernel is power limited).  The two rows in use and the one or two being fetched are always in different
//   slots; the odd stage still issues its patch pieces only behind the barrier that follows the straddling pair.  The
//   fragment bases become per-couple values (a dozen vector adds per 3 432 matrix instructions).
//   Measured (one box, inside the train step): block 2 / 3 / 4 forward 12.24 -> 11.77 / 5.92 -> 5.72 / 2.96 -> 2.88 ms.
template <int T, bool RING>       // RING is always true: the kernel keeps the name the profiles and bench.py's roofline block know it by
__global__ __launch_bounds__(256, 1) void conv_f16x3_dma16_kernel(ConvF16Args a)
{
    static_assert(RING, "the four-row ring is the only patch scheme");
    constexpr int NCB = 4, NKH = CV_KH;
    // Plane pitch of the patch images, in positions.  A B fragment of this kernel is read by lane groups (tap parity, k half): the
    // hardware serves a ds_read_b128 sixteen lanes at a time -- eight lanes of k half 0 and eight of k half 1 -- and with 352 + 12 T
    // positions per plane (5 824 / 6 016 bytes at T = 1 / 2: 192 / 128 mod 256) the two halves of a group met on the same banks:
    // every patch-fragment read took twice its cycles (SQ_LDS_BANK_CONFLICT = 43 % of the kernel's LDS cycles at T = 1, 2 and 0.2 %
    // at T = 4, whose 6 400-byte planes are a multiple of 256: profiles/r05/pmc_b64_lds.txt).  Rounded up to a multiple of 16
    // positions every plane starts on bank 0 -- the extra positions are halo (zeros) and fit the same number of DMA pieces.
    constexpr int PWP = (CV_PITCH + 12 * T + 15) / 16 * 16;
    constexpr int WSL = CV_KW * 64 * 16;
    constexpr int PLANE = PWP * 16;
    constexpr int W_SPLIT = 7 * 2048, W_BYTES = 2 * W_SPLIT;
    constexpr int N_STAGE = NCB * NKH;
    static_assert(N_STAGE % 2 == 0, "DMA schedule");
    constexpr int R_PIECES = (4 * PWP + 63) / 64;                // pieces of one patch row = 4 planes [split][khalf]
    constexpr int SLOT_BYTES = R_PIECES * 1024;
    constexpr int RPW = (R_PIECES + 3) / 4;                      //       per wave
    static_assert(RPW >= 6 && RPW <= 7, "DMA schedule");
    constexpr int SP_STRIDE = 2 * PLANE;                         // bytes between the hi and lo images of a patch row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int W0_OFF = 0, W1_OFF = W_BYTES, P0_OFF = 2 * W_BYTES;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = wave >> 1, c = wave & 1, g = lane >> 4, l16 = lane & 15, tp = g >> 1, khf = g & 1;
    int tile_id = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const int n_tiles = gridDim.x * gridDim.y;
        if ((n_tiles & 7) == 0) tile_id = (tile_id & 7) * (n_tiles >> 3) + (tile_id >> 3);
    }
    const int b = tile_id / gridDim.x, h0 = (tile_id - b * gridDim.x) * 2;

    floatx4 acc[44];
#pragma unroll
    for (int i = 0; i < 44; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][r] = 0.0f;

    // patch piece descriptors of one row: bit 31 = no source (halo column / padding slot), bit 30 = split, low bits = byte offset
    // of the slot's 16 bytes inside the operand row
    int desc[RPW];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = (wave + 4 * k) * 64 + lane;
        const int plane = i / PWP, pos = i - plane * PWP, w = pos - 6 * T;
        const int split = plane >> 1, part = plane & 1;
        desc[k] = (i < 4 * PWP && w >= 0 && w < CV_PITCH) ? ((split << 30) | (w * 32 + part * 16)) : -1;
    }
    const unsigned long long zero_src = (unsigned long long)k_zero_slot, xh = (unsigned long long)a.x_hi,
                             xl = (unsigned long long)a.x_lo, wh = (unsigned long long)a.w_hi, wlo = (unsigned long long)a.w_lo;
    const int H = a.H;

    struct DmaSlot { unsigned long long src; unsigned lds; };
    // weights of (stage, taps [t0, t0 + nt)) -> tap slots 0.. of the buffer at woff; piece pw covers one (split, tap, khalf) plane
    auto slot_w = [&](int st, int t0, int nt, int woff, int j) {
        const int pw = wave + 4 * j, per = 2 * nt;
        const int split = pw / per, rem = pw - split * per;
        DmaSlot d;
        d.src = (split ? wlo : wh) + ((unsigned long long)st * WSL + (t0 * 2 + rem) * 512 + lane * 8) * 2;
        d.lds = lds0 + woff + split * W_SPLIT + rem * 1024;
        return d;
    };
    // piece k of input row j (= h0 - 2 + j) of channel block cb -> row slot (6 cb + j) & 3; cb == NCB: zeros (no next stage)
    auto slot_row = [&](int cb, int j, int k) {
        const bool in_range = wave + 4 * k < R_PIECES;
        const int pp = in_range ? wave + 4 * k : wave + 4 * (k - 1);
        const int d = in_range ? desc[k] : desc[k > 0 ? k - 1 : 0];
        const int hx = h0 + j - NKH / 2;
        const bool v = hx >= 0 && hx < H && cb < NCB;
        const long long st_off = (((long long)b * H + hx) * NCB + cb) * (CV_PITCH * 32);
        const unsigned long long src = ((d & (1 << 30)) ? xl : xh) + st_off + (unsigned)(d & 0xFFFFF);
        DmaSlot r;
        r.src = (d >= 0 && v) ? src : zero_src;
        r.lds = lds0 + P0_OFF + ((cb * 6 + j) & 3) * SLOT_BYTES + pp * 1024;
        return r;
    };
    auto slot_issue = [&](const DmaSlot &d) { glds16(d.src, d.lds); };
    auto row_burst = [&](int cb, int j) {                    // a whole row at once (the second new row of a stage that opens a channel block)
#pragma unroll
        for (int k = 0; k < RPW; ++k)
            if (wave + 4 * k < R_PIECES) slot_issue(slot_row(cb, j, k));
    };

    // prologue: taps 0..5 of stage 0 and its patch
#pragma unroll
    for (int j = 0; j < 6; ++j) slot_issue(slot_w(0, 0, 6, W0_OFF, j));
    row_burst(0, 0);
    row_burst(0, 1);
    DMA_WAIT();
    __syncthreads();

    // lane parts of the fragment addresses.  A = weights of channel half hh ^ c (hh relative to the wave), B = patch.
    //   regular pair : + buffer offset + split * W_SPLIT + first tap slot * 2048 + (ct & 1) * 256   /   + row slot + nt * 256 + kw * T * 16 + split * SP_STRIDE
    //   straddling   : parity-0 lanes -> tap slot 6 of W1 / tap 12 of the even stage's row, parity-1 lanes -> tap slot 0 of W0 / tap 0 of the odd stage's row
    const int a_k = khf * 1024 + l16 * 16, b_k = khf * PLANE + l16 * 16;
    const unsigned char *const a_p0 = smem + a_k + tp * 2048 + c * 512, *const a_p1 = smem + a_k + tp * 2048 + (c ^ 1) * 512;
    // patch fragment bases of the even / odd stage and of the straddling pair: re-based per stage couple below (the rows move round the ring)
    const unsigned char *b_pE, *bm_pE, *b_pO, *bm_pO, *bs_p, *bsm_p;
    const int b_x = (c * 6 * 32 + tp * T) * 16, bm_x = (5 * 32 + tp * T) * 16;      // column parts of the regular pairs' bases
    const int sa_off = tp ? W0_OFF : W1_OFF + 6 * 2048;
    const unsigned char *const as_p0 = smem + a_k + sa_off + c * 512, *const as_p1 = smem + a_k + sa_off + (c ^ 1) * 512;

    // fragments: A double buffered [buf][ctr * 2 + split] (ctr = channel tile relative to the wave: 0, 1 = half c), B ring [slot][split]
    // with slot = nt % 6 for column tile nt < 10 and 4, 5 for the middle tile's halves 10, 11
    half8 FA[2][8], FB[6][2];
    auto rdA = [&](int buf, int woff, int tl, int q) {
        const int ctr = q >> 1, sp = q & 1;
        FA[buf][q] = *reinterpret_cast<const half8 *>(((ctr >> 1) ? a_p1 : a_p0) + woff + sp * W_SPLIT + tl * 2048 + (ctr & 1) * 256);
    };
    auto rdB = [&](int odd, int kw, int nt, int sp) {
        FB[nt < 10 ? nt % 6 : nt - 6][sp] = *reinterpret_cast<const half8 *>(
            (nt < 10 ? (odd ? b_pO : b_pE) + nt * 256 : (odd ? bm_pO : bm_pE) + (nt - 10) * 256) + kw * T * 16 + sp * SP_STRIDE);
    };
    auto rdA_str = [&](int buf, int q) {
        const int ctr = q >> 1, sp = q & 1;
        FA[buf][q] = *reinterpret_cast<const half8 *>(((ctr >> 1) ? as_p1 : as_p0) + sp * W_SPLIT + (ctr & 1) * 256);
    };
    auto rdB_str = [&](int nt, int sp) {
        FB[nt < 10 ? nt % 6 : nt - 6][sp] =
            *reinterpret_cast<const half8 *>((nt < 10 ? bs_p + nt * 256 : bsm_p + (nt - 10) * 256) + sp * SP_STRIDE);
    };
    // instruction m (0..11) of group gi of a pair; gi < 10: column tile gi x 4 channel tiles; gi == 10: tiles 10, 11 x 2
    // channel tiles; term-major, so one accumulator every 4th instruction.  Written as inline assembly with the
    // accumulator TIED (dest = src C, AGPR): the builtin leaves dest and src C of this 4-pass shape independent, the
    // allocator renamed a third of them and paid for it with ~90 v_accvgpr moves per stage at the loop edge.  Inline
    // assembly is opaque to the scheduler, so the MFMA / ds_read interleave below is pinned by sched_barrier fences in
    // source order; the waits for the fragment reads are still the compiler's (register operands of the asm).
    auto mma1 = [&](int buf, int gi, int m) {
        const int term = m >> 2, q = m & 3;
        const int nt = gi < 10 ? gi : 10 + (q >> 1), ctr = gi < 10 ? q : (q & 1);
        const int u = gi < 10 ? gi * 4 + q : 40 + q;
        const half8 av = FA[buf][ctr * 2 + (term == 0 ? 1 : 0)];
        const half8 bv = FB[nt < 10 ? nt % 6 : nt - 6][term == 1 ? 1 : 0];
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc[u]) : "v"(av), "v"(bv));
    };
    // One group = 12 instructions on A buffer BUF.  Reads in its shadow, four tiles ahead:
    //   groups 0..5: column tile gi + 4 of THIS pair (RDB_CUR(nt, split));  group 6: its tiles 10, 11;
    //   groups 7..10: tile gi - 7 of the NEXT pair (RDB_NXT) if NB;  groups 0..7: A fragment gi of the next pair (RDA_NXT(buf, q)) if NA.
    // then NS (<= 2) DMA pieces.
#define DMA16_GROUP(BUF, GI, RDB_CUR, NA, RDA_NXT, NB, RDB_NXT, NS, SLOT_1, SLOT_2)                  \
    {                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        const DmaSlot s1_ = SLOT_1, s2_ = SLOT_2;                                                      \
        constexpr int nb_ = (GI) < 6 ? 2 : (GI) == 6 ? 4 : (NB) ? 2 : 0;      /* patch reads, then the A read */ \
        constexpr int nr_ = nb_ + (((NA) && (GI) < 8) ? 1 : 0);                                        \
        constexpr int every_ = nr_ == 0 ? 99 : nr_ == 1 ? 6 : nr_ == 2 ? 4 : nr_ == 3 ? 3 : 2;         \
        _Pragma("unroll") for (int m_ = 0; m_ < 12; ++m_) {                                            \
            mma1(BUF, GI, m_);                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                         \
            if ((m_ + 1) % every_ == 0 && (m_ + 1) / every_ <= nr_) {                                  \
                const int j_ = (m_ + 1) / every_ - 1;                                                  \
                if (j_ < nb_) {                                                                        \
                    if ((GI) < 6) { RDB_CUR((GI) + 4, j_); }                                           \
                    else if ((GI) == 6) { RDB_CUR(10 + (j_ >> 1), j_ & 1); }                           \
                    else { RDB_NXT((GI) - 7, j_); }                                                    \
                } else {                                                                               \
                    RDA_NXT((BUF) ^ 1, GI);                                                            \
                }                                                                                      \
                __builtin_amdgcn_sched_barrier(0);                                                     \
            }                                                                                          \
        }                                                                                              \
        if ((NS) >= 1) slot_issue(s1_);                                                                \
        if ((NS) >= 2) slot_issue(s2_);                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                             \
    }
    // groups 2, 5, 8, 10 of a pair carry its DMA slots SBASE + 0..3; the others none
#define DMA16_G_(BUF, GI, RC, NA, RA, NB, RN) DMA16_GROUP(BUF, GI, RC, NA, RA, NB, RN, 0, DmaSlot{}, DmaSlot{})
#define DMA16_S_(BUF, GI, RC, NA, RA, NB, RN, SLOTN, SLOT_A, SLOT_B, SL) DMA16_GROUP(BUF, GI, RC, NA, RA, NB, RN, SLOTN(SL), SLOT_A(SL), SLOT_B(SL))
#define DMA16_PAIR(BUF, RC, NA, RA, NB, RN, SLOTN, SLOT_A, SLOT_B, SBASE)                 \
    DMA16_G_(BUF, 0, RC, NA, RA, NB, RN)                                                  \
    DMA16_G_(BUF, 1, RC, NA, RA, NB, RN)                                                  \
    DMA16_S_(BUF, 2, RC, NA, RA, NB, RN, SLOTN, SLOT_A, SLOT_B, (SBASE) + 0)              \
    DMA16_G_(BUF, 3, RC, NA, RA, NB, RN)                                                  \
    DMA16_G_(BUF, 4, RC, NA, RA, NB, RN)                                                  \
    DMA16_S_(BUF, 5, RC, NA, RA, NB, RN, SLOTN, SLOT_A, SLOT_B, (SBASE) + 1)              \
    DMA16_G_(BUF, 6, RC, NA, RA, NB, RN)                                                  \
    DMA16_G_(BUF, 7, RC, NA, RA, NB, RN)                                                  \
    DMA16_S_(BUF, 8, RC, NA, RA, NB, RN, SLOTN, SLOT_A, SLOT_B, (SBASE) + 2)              \
    DMA16_G_(BUF, 9, RC, NA, RA, NB, RN)                                                  \
    DMA16_S_(BUF, 10, RC, NA, RA, NB, RN, SLOTN, SLOT_A, SLOT_B, (SBASE) + 3)
    // fragment readers of the schedule below: patch of the even stage (b_pE), of the odd stage (b_pO), of the straddling pair
#define RB_E(KW) [&](int nt_, int sp_) { rdB(0, KW, nt_, sp_); }
#define RB_O(KW) [&](int nt_, int sp_) { rdB(1, KW, nt_, sp_); }
#define RB_S [&](int nt_, int sp_) { rdB_str(nt_, sp_); }
#define RA_(WOFF, TL) [&](int buf_, int q_) { rdA(buf_, WOFF, TL, q_); }
#define R_NONE [&](int, int) {}

#pragma unroll 1
    for (int s = 0; s < N_STAGE; s += 2) {
        const int so = s + 1, sn = s + 2 < N_STAGE ? s + 2 : s + 1;      // odd stage; the stage after it (last couple: harmless repeats)
        // the new rows of the odd stage (fetched during the even one) and of stage s + 2 (fetched during the odd one):
        // row A = kernel row + 1 of the successor, always; row B = its row 0, only when it opens a channel block
        const int cbo = so / NKH, kho = so - cbo * NKH, cbn = (s + 2) / NKH, khn = (s + 2) - cbn * NKH;
        const bool two_e = kho == 0, two_o = khn == 0 && s + 2 < N_STAGE;
        {
            const int n0e = (s / NKH) * 6 + s % NKH + row, n0o = cbo * 6 + kho + row;
            const int oe = P0_OFF + (n0e & 3) * SLOT_BYTES, oo = P0_OFF + (n0o & 3) * SLOT_BYTES;
            b_pE = smem + oe + b_k + b_x;
            bm_pE = smem + oe + b_k + bm_x;
            b_pO = smem + oo + b_k + b_x;
            bm_pO = smem + oo + b_k + bm_x;
            const int os = tp ? oo : oe + 12 * T * 16;
            bs_p = smem + b_k + os + c * 6 * 32 * 16;
            bsm_p = smem + b_k + os + 5 * 32 * 16;
        }
        // ================= even stage s: taps 0..11 (W0 = taps 0..5, W1 = taps 6..12) =================
        // DMA phase A (12 slots): W1 <- taps 6..12 of s in slots 0..6, pieces 0..4 of the odd stage's new row in slots 7..11; ends on vmcnt(5)
        //     phase B (12 slots): W0 <- taps 0..6 of s + 1 in slots 0..6 with the row's pieces 5.. riding along
#define EA_SLOTN(J) 1
#define PATCH_E_(K) slot_row(cbo, kho + 1, (K))
#define PATCH_O_(K) slot_row(cbn, khn + 1, (K))
#define EA_SLOT1(J) ((J) < 7 ? slot_w(s, 6, 7, W1_OFF, (J)) : PATCH_E_((J) - 7))
#define EB_SLOTN(J) (((J) < 7 ? 1 : 0) + ((J) + 5 < RPW ? 1 : 0))
#define EB_SLOT1(J) ((J) < 7 ? slot_w(so, 0, 7, W0_OFF, (J)) : PATCH_E_((J) + 5 < RPW ? (J) + 5 : RPW - 1))
#define EB_SLOT2(J) PATCH_E_((J) + 5 < RPW ? (J) + 5 : RPW - 1)
#pragma unroll
        for (int q = 0; q < 8; ++q) rdA(0, W0_OFF, 0, q);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) { rdB(0, 0, nt, 0); rdB(0, 0, nt, 1); }
        DMA16_PAIR(0, RB_E(0), 1, RA_(W0_OFF, 2), 1, RB_E(2), EA_SLOTN, EA_SLOT1, EA_SLOT1, 0)
        DMA16_PAIR(1, RB_E(2), 1, RA_(W0_OFF, 4), 1, RB_E(4), EA_SLOTN, EA_SLOT1, EA_SLOT1, 4)
        DMA16_PAIR(0, RB_E(4), 0, R_NONE, 1, RB_E(6), EA_SLOTN, EA_SLOT1, EA_SLOT1, 8)          // W1 is not there yet
        asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) rdA(1, W1_OFF, 0, q);
        if (two_e) row_burst(cbo, 0);
        DMA16_PAIR(1, RB_E(6), 1, RA_(W1_OFF, 2), 1, RB_E(8), EB_SLOTN, EB_SLOT1, EB_SLOT2, 0)
        DMA16_PAIR(0, RB_E(8), 1, RA_(W1_OFF, 4), 1, RB_E(10), EB_SLOTN, EB_SLOT1, EB_SLOT2, 4)
        DMA16_PAIR(1, RB_E(10), 0, R_NONE, 0, R_NONE, EB_SLOTN, EB_SLOT1, EB_SLOT2, 8)          // the next pair straddles: its operands land with the barrier
        DMA_WAIT();
        __syncthreads();
        // ================= odd stage s + 1: the straddling pair, then taps 1..12 (W0 = taps 0..6, W1 = taps 7..12) =====
        // DMA phase A (16 slots): W1 <- taps 7..12 of s + 1 in slots 0..5 (tap slot 6 of W1 keeps the even stage's tap 12);
        //                         after the barrier behind the straddling pair: pieces 0..5 of stage s + 2's new row in slots 6..11;
        //                         ends on vmcnt(6)
        //     phase B (12 slots): W0 <- taps 0..5 of s + 2 in slots 0..5 with the row's piece 6 riding along
#define OA_SLOTN(J) ((J) < 12 ? 1 : 0)
#define OA_SLOT1(J) ((J) < 6 ? slot_w(so, 7, 6, W1_OFF, (J)) : PATCH_O_((J) < 12 ? (J) - 6 : 5))
#define OB_SLOTN(J) (((J) < 6 ? 1 : 0) + ((J) + 6 < RPW ? 1 : 0))
#define OB_SLOT1(J) ((J) < 6 ? slot_w(sn, 0, 6, W0_OFF, (J)) : PATCH_O_((J) + 6 < RPW ? (J) + 6 : RPW - 1))
#define OB_SLOT2(J) PATCH_O_((J) + 6 < RPW ? (J) + 6 : RPW - 1)
#pragma unroll
        for (int q = 0; q < 8; ++q) rdA_str(0, q);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) { rdB_str(nt, 0); rdB_str(nt, 1); }
        DMA16_PAIR(0, RB_S, 1, RA_(W0_OFF, 1), 1, RB_O(1), OA_SLOTN, OA_SLOT1, OA_SLOT1, 0)     // slots 0..3: weights only
        if (!(DMA16_ABL & 2)) __builtin_amdgcn_s_barrier();   // every wave holds the straddling pair's operands: patch pieces may be issued from here on
        DMA16_PAIR(1, RB_O(1), 1, RA_(W0_OFF, 3), 1, RB_O(3), OA_SLOTN, OA_SLOT1, OA_SLOT1, 4)
        DMA16_PAIR(0, RB_O(3), 1, RA_(W0_OFF, 5), 1, RB_O(5), OA_SLOTN, OA_SLOT1, OA_SLOT1, 8)
        DMA16_PAIR(1, RB_O(5), 0, R_NONE, 1, RB_O(7), OA_SLOTN, OA_SLOT1, OA_SLOT1, 12)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) rdA(0, W1_OFF, 0, q);
        if (two_o) row_burst(cbn, 0);
        DMA16_PAIR(0, RB_O(7), 1, RA_(W1_OFF, 2), 1, RB_O(9), OB_SLOTN, OB_SLOT1, OB_SLOT2, 0)
        DMA16_PAIR(1, RB_O(9), 1, RA_(W1_OFF, 4), 1, RB_O(11), OB_SLOTN, OB_SLOT1, OB_SLOT2, 4)
        DMA16_PAIR(0, RB_O(11), 0, R_NONE, 0, R_NONE, OB_SLOTN, OB_SLOT1, OB_SLOT2, 8)
        DMA_WAIT();
        __syncthreads();
    }
#undef DMA16_GROUP
#undef DMA16_G_
#undef DMA16_S_
#undef DMA16_PAIR
#undef RB_E
#undef RB_O
#undef RB_S
#undef RA_
#undef R_NONE
#undef EA_SLOTN
#undef EA_SLOT1
#undef EB_SLOTN
#undef EB_SLOT1
#undef EB_SLOT2
#undef OA_SLOTN
#undef OA_SLOT1
#undef OB_SLOTN
#undef OB_SLOT1
#undef OB_SLOT2
#undef PATCH_E_
#undef PATCH_O_
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");           // the asm MFMAs are invisible to the hazard recogniser: results settled before the epilogue reads them
    conv_f16_epilogue<0>(acc, a, smem, b, h0, row, c, lane);
}

// ---- LDS-DMA version on a ring of THREE row slots (forward, T = 8 and 16) --------------------------------------------
// conv_f16x3_dma_kernel's tap body (v_mfma_f32_32x32x16_f16: K = one tap x 16 channels, so no tap pair straddles two
// stages and no more than two patch rows are ever read at once), weights in the same two half-stage buffers, the patch in
// a ring of three ROW slots of 4 planes [split][khalf] x (352 + 12 T) positions:
//   T = 8 : 2 x 28 KB + 3 x 28 672 B = 143 360 B;      T = 16 : 2 x 28 KB + 3 x 34 816 B = 161 792 B (budget 163 840).
// The plane pitches (448 / 544 positions) are multiples of 16 positions: every plane starts on bank 0.
// Stage (cb, kh) reads input rows j = kh (output row 0) and kh + 1 (output row 1) of the six rows j = 0..5 = h0 - 2 ..
// h0 + 3 of channel block cb; row j lives in slot j % 3 (6 cb + j = j mod 3).  The stage fetches row kh + 2 for its
// successor into the slot that row kh - 1 left; stage (cb, 4) fetches row 0 of block cb + 1 into the free slot 0, and
// row 1 of that block -- slot 1 holds row 4 until the stage ends -- follows the end-of-stage barrier in one burst: one
// exposed row fetch per channel-block opening, three per workgroup.  (A stage order that avoids it would have to change
// the order in which an accumulator meets its stages, and with it the rounding: results stay bit-identical instead.)
// DMA pieces per wave and stage: 6 + 7 of weights, 7 (T = 8) / 9 (T = 16) of the new row, in the 26 slots of a stage:
//   phase A (14 slots): W1 <- this stage's taps 7..12 in slots 0..5, row pieces 0..7 behind them; ends on vmcnt(row pieces)
//   phase B (12 slots): W0 <- the next stage's taps 0..6 in slots 0..6, row piece 8 riding along in slot 0; ends on vmcnt(0)
//
// Halo tiles.  The B fragment of (tap kw, column tile nt) holds patch positions 32 nt + l + kw T, l < 32, that is image
// columns w = 32 nt + l + (kw - 6) T.  Positions with w < 0 or w >= 352 are never fetched from the operand: their DMA
// descriptor names the zero slot (make of desc[] below), whatever Wv is and whatever the operand's pad columns hold.  So
// the fragment is all zeros, for EVERY frame count, exactly when 32 nt + 31 + (kw - 6) T < 0 or 32 nt + (kw - 6) T >= 352
// (conv_halo_tile): its three matrix instructions per channel half add products with an exact zero operand, and they and the
// fragment's two LDS reads are left out.  T = 16: left nt = 0 for kw <= 4, nt = 1 for kw <= 2, nt = 2 for kw = 0, and
// mirrored on the right (nt = 10, 9, 8 for kw >= 8, 10, 12): 18 of the 143 (tap, tile) pairs; T = 8: nt = 0 for kw <= 2
// and nt = 10 for kw >= 10: 6 of 143.  (With the shipped 345 frames the set is the same: the next candidate, nt = 10 at
// shift 16, still reaches column 336 < 345.)  One instantiation therefore serves every Wv.  The taps are unrolled, so
// the set is a compile-time property of (tap, tile, column half); the K loop is instantiated once per column half and the
// wave-uniform c selects the instance once (k_loop below), so every tap is straight-line code; tile 5 (both halves) is
// never in the set.  (Choosing between two bodies per TAP spilled 385 / 950 registers: every tap then ends in a join of
// fragment sets of which only one side wrote the halo tiles'.)  Measured: profiles/r22/README.md.
__host__ __device__ constexpr bool conv_halo_tile(int T, int kw, int nt)
{
    return 32 * nt + 31 + (kw - 6) * T < 0 || 32 * nt + (kw - 6) * T >= CV_PITCH;
}

#ifndef DMA3_SKIP
#define DMA3_SKIP 1     // 0: every halo tile computed (for A/B timing; same results)
#endif
template <int T>
__global__ __launch_bounds__(256, 1) void conv_f16x3_dma3_kernel(ConvF16Args a)
{
    constexpr int NCB = 4, NKH = CV_KH;
    constexpr int PWP = CV_PITCH + 12 * T;            // patch positions per row (w = q - 6T)
    static_assert(PWP % 16 == 0, "plane pitch: a multiple of 16 positions, so that every row is whole DMA pieces on bank 0");
    constexpr int WSL = CV_KW * 64 * 16;
    constexpr int PLANE = PWP * 16;                   // bytes of one (split, khalf) plane of a row
    constexpr int W_SPLIT = 7 * 2048, W_BYTES = 2 * W_SPLIT;
    constexpr int R_PIECES = 4 * PWP / 64;            // pieces of one patch row = 4 planes [split][khalf]: 28 / 34
    constexpr int SLOT_BYTES = R_PIECES * 1024;
    constexpr int RPW = (R_PIECES + 3) / 4;           //        per wave: 7 / 9
    constexpr int RPA = RPW < 8 ? RPW : 8;            //        of them in phase A
    static_assert(RPW >= 7 && RPW <= 9, "DMA schedule");
    constexpr int SP_STRIDE = 2 * PLANE;              // bytes between the hi and lo images of a patch row
    constexpr int W0_OFF = 0, W1_OFF = W_BYTES, P0_OFF = 2 * W_BYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = wave >> 1, c = wave & 1, half = lane >> 5, l32 = lane & 31;
    // XCD-contiguous (clip, row pair) tiles: see conv_f16x3_kernel
    int tile_id = blockIdx.y * gridDim.x + blockIdx.x;
    {
        const int n_tiles = gridDim.x * gridDim.y;
        if ((n_tiles & 7) == 0) tile_id = (tile_id & 7) * (n_tiles >> 3) + (tile_id >> 3);
    }
    const int b = tile_id / gridDim.x, h0 = (tile_id - b * gridDim.x) * 2;

    floatx16 acc[CV_WT];
#pragma unroll
    for (int i = 0; i < CV_WT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    // patch piece descriptors of one row: bit 31 = no source (halo column), bit 30 = split, low bits = byte offset of the
    // slot's 16 bytes inside the operand row
    int desc[RPW];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int i = (wave + 4 * k) * 64 + lane;
        const int plane = i / PWP, pos = i - plane * PWP, w = pos - 6 * T;
        const int split = plane >> 1, part = plane & 1;
        desc[k] = (i < 4 * PWP && w >= 0 && w < CV_PITCH) ? ((split << 30) | (w * 32 + part * 16)) : -1;
    }
    const unsigned long long zero_src = (unsigned long long)k_zero_slot, xh = (unsigned long long)a.x_hi,
                             xl = (unsigned long long)a.x_lo, wh = (unsigned long long)a.w_hi, wlo = (unsigned long long)a.w_lo;
    const int H = a.H;

    // DMA slots: issued unconditionally, address arithmetic apart from the issue (see conv_f16x3_dma_kernel)
    struct DmaSlot { unsigned long long src; unsigned lds; };
    auto slot_w = [&](int st, int t0, int nt, int woff, int j) {
        const int pw = wave + 4 * j, per = 2 * nt;
        const int split = pw / per, rem = pw - split * per;
        DmaSlot d;
        d.src = (split ? wlo : wh) + ((unsigned long long)st * WSL + (t0 * 2 + rem) * 512 + lane * 8) * 2;
        d.lds = lds0 + woff + split * W_SPLIT + rem * 1024;
        return d;
    };
    // piece k of input row j (= h0 - 2 + j) of channel block cb -> row slot j % 3; cb == NCB: zeros (no next stage);
    // a wave without a piece k repeats its piece k - 1 (the same bytes to the same place)
    auto slot_row = [&](int cb, int j, int k) {
        const bool in_range = wave + 4 * k < R_PIECES;
        const int pp = in_range ? wave + 4 * k : wave + 4 * (k - 1);
        const int d = in_range ? desc[k] : desc[k > 0 ? k - 1 : 0];
        const int hx = h0 + j - NKH / 2;
        const bool v = hx >= 0 && hx < H && cb < NCB;
        const long long st_off = (((long long)b * H + hx) * NCB + cb) * (CV_PITCH * 32);
        const unsigned long long src = ((d & (1 << 30)) ? xl : xh) + st_off + (unsigned)(d & 0xFFFFF);
        DmaSlot r;
        r.src = (d >= 0 && v) ? src : zero_src;
        r.lds = lds0 + P0_OFF + (j % 3) * SLOT_BYTES + pp * 1024;
        return r;
    };
    auto slot_issue = [&](const DmaSlot &d) { glds16(d.src, d.lds); };
    auto row_burst = [&](int cb, int j) {                    // a whole row at once
#pragma unroll
        for (int k = 0; k < RPW; ++k)
            if (wave + 4 * k < R_PIECES) slot_issue(slot_row(cb, j, k));
    };

    // prologue: taps 0..6 of stage 0 and its two rows
#pragma unroll
    for (int j = 0; j < 7; ++j) slot_issue(slot_w(0, 0, 7, W0_OFF, j));
    row_burst(0, 0);
    row_burst(0, 1);
    DMA_WAIT();
    __syncthreads();

    // The K loop for column half C (C < 0: no tile counts as halo), instantiated once per column half: the halo set is
    // then a compile-time property of every tap's straight-line body, and the wave-uniform c selects the instance ONCE.
    // Both instances execute the same sequence of workgroup barriers.
    auto k_loop = [&](auto c_tag) __attribute__((always_inline)) {
    constexpr int C = decltype(c_tag)::value;
#pragma unroll 1
    for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll 1
        for (int kh = 0; kh < NKH; ++kh) {
            const int s = cb * NKH + kh;
            const bool more = s + 1 < NCB * NKH;
            const int sn = more ? s + 1 : s;             // the stage whose weights the phase-B slots fetch (last stage: its own again, into the buffer nobody reads any more)
            // the row fetched for the successor: its kernel row + 1, or row 0 when it opens a channel block (cbn == NCB: zeros)
            const int cbn = kh + 1 < NKH ? cb : cb + 1, jn = kh + 1 < NKH ? kh + 2 : 0;
            const unsigned char *const Pr = smem + P0_OFF + ((kh + row) % 3) * SLOT_BYTES;       // this wave's input row
            const unsigned char *b_p = Pr + half * PLANE + (c * 6 * 32 + l32) * 16;              // + split*SP_STRIDE + (t*32 + kw*T)*16
            const unsigned char *bm_p = Pr + half * PLANE + (5 * 32 + l32) * 16;                 // middle tile
            // fragments of one tap, double buffered (FA: a0h a0l a1h a1l; FBH/FBL: tiles 0..4 + the middle tile)
            half8 FA[2][4], FBH[2][6], FBL[2][6];
            // column tile of the wave's patch fragment `tile` for column half C; C < 0: no tile counts as halo
            auto halo = [&](int C, int kw, int tile) { return C >= 0 && conv_halo_tile(T, kw, tile < 5 ? C * 6 + tile : 5); };
            // read r (0..15) of the tap (weights buffer at woff, local tap tl, kernel column kw) into fragment set f
            auto rd = [&](int C, int f, int woff, int tl, int kw, int r) {
                if (r < 4) {
                    const int ch = (r >> 1) ? (c ^ 1) : c;
                    FA[f][r] = *reinterpret_cast<const half8 *>(smem + woff + (r & 1) * W_SPLIT + (tl * 2 + half) * 1024 + (ch * 32 + l32) * 16);
                } else {
                    const int tile = (r - 4) >> 1, lo = (r - 4) & 1;
                    if (halo(C, kw, tile)) return;
                    const unsigned char *p = (tile < 5 ? b_p + tile * 32 * 16 : bm_p) + lo * SP_STRIDE + kw * T * 16;
                    if (lo) FBL[f][tile] = *reinterpret_cast<const half8 *>(p);
                    else FBH[f][tile] = *reinterpret_cast<const half8 *>(p);
                }
            };
            // MFMA i (0..32) of tap kw: term (lo*hi, hi*lo, hi*hi) x 11 accumulators
            auto mma = [&](int C, int f, int kw, int i) {
                const int term = i / 11, u = i - term * 11;
                const int tile = u < 10 ? (u >> 1) : 5, j = u < 10 ? (u & 1) : 0;
                if (halo(C, kw, tile)) return;
                const half8 av = FA[f][2 * j + (term == 0 ? 1 : 0)];
                const half8 bv = term == 1 ? FBL[f][tile] : FBH[f][tile];
                acc[u] = mfma16(av, bv, acc[u]);
            };
            // One tap for column half C: its MFMAs on set F, the next tap's fragment reads into set F^1 (r_lo..15), one read
            // after every second MFMA, pinned, and two DMA slots (see conv_f16x3_dma_kernel)
#define DMA3_TAP_C(C, F, WOFF, TLN, KW, KWN, R_LO, NA, SLOT_A, SLOT_A2, NB, SLOT_B, SLOT_B2)              \
    {                                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        const DmaSlot sa_ = SLOT_A, sa2_ = SLOT_A2;                                                      \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) mma(C, F, KW, i);                                 \
        _Pragma("unroll") for (int r = 0; r < 8; ++r) if (r >= (R_LO)) rd(C, (F) ^ 1, WOFF, TLN, KWN, r); \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                                  \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                           \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                           \
        }                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        if ((NA) >= 1) slot_issue(sa_);                                                                  \
        if ((NA) >= 2) slot_issue(sa2_);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        const DmaSlot sb_ = SLOT_B, sb2_ = SLOT_B2;                                                      \
        _Pragma("unroll") for (int i = 16; i < 33; ++i) mma(C, F, KW, i);                                \
        _Pragma("unroll") for (int r = 8; r < 16; ++r) if (r >= (R_LO)) rd(C, (F) ^ 1, WOFF, TLN, KWN, r); \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                                  \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                           \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                           \
        }                                                                                                \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                               \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        if ((NB) >= 1) slot_issue(sb_);                                                                  \
        if ((NB) >= 2) slot_issue(sb2_);                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
    }
#define DMA3_TAP(...) DMA3_TAP_C(C, __VA_ARGS__)
#define DMA3_ROW(K) slot_row(cbn, jn, (K) < RPW ? (K) : RPW - 1)
#define DMA3_NA(J) ((J) < 6 + RPA ? 1 : 0)
#define DMA3_SLOT_A(J) ((J) < 6 ? slot_w(s, 7, 6, W1_OFF, (J)) : DMA3_ROW((J) - 6))
#define DMA3_NB(J) (((J) < 7 ? 1 : 0) + ((J) + 8 < RPW ? 1 : 0))
#define DMA3_SLOT_B(J) slot_w(sn, 0, 7, W0_OFF, (J) < 7 ? (J) : 0)
#define DMA3_SLOT_B2(J) DMA3_ROW((J) + 8)

            // ---- phase A: taps 0..6 from W0 (tap 0's fragments: all of them, halo tiles included -- once per stage)
#pragma unroll
            for (int r = 0; r < 16; ++r) rd(-1, 0, W0_OFF, 0, 0, r);
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                if (t < 6) DMA3_TAP(t & 1, W0_OFF, t + 1, t, t + 1, 0, DMA3_NA(2 * t), DMA3_SLOT_A(2 * t), DMA3_SLOT_A(2 * t), DMA3_NA(2 * t + 1), DMA3_SLOT_A(2 * t + 1), DMA3_SLOT_A(2 * t + 1))
                else DMA3_TAP(t & 1, W0_OFF, 0, t, 7, 4, DMA3_NA(2 * t), DMA3_SLOT_A(2 * t), DMA3_SLOT_A(2 * t), DMA3_NA(2 * t + 1), DMA3_SLOT_A(2 * t + 1), DMA3_SLOT_A(2 * t + 1))     // tap 7's patch fragments only
            }
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RPA) : "memory");     // this wave's W1 pieces landed (the row pieces behind them may be in flight) ...
            __syncthreads();                                               // ... and everyone's did
            // ---- phase B: taps 7..12 from W1 (fragment set 1 holds tap 7's patch fragments)
#pragma unroll
            for (int r = 0; r < 4; ++r) rd(-1, 1, W1_OFF, 0, 7, r);
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                if (t < 5) DMA3_TAP((t + 1) & 1, W1_OFF, t + 1, 7 + t, 8 + t, 0, DMA3_NB(2 * t), DMA3_SLOT_B(2 * t), DMA3_SLOT_B2(2 * t), DMA3_NB(2 * t + 1), DMA3_SLOT_B(2 * t + 1), DMA3_SLOT_B2(2 * t + 1))
                else DMA3_TAP((t + 1) & 1, W1_OFF, 0, 7 + t, 0, 16, DMA3_NB(2 * t), DMA3_SLOT_B(2 * t), DMA3_SLOT_B2(2 * t), DMA3_NB(2 * t + 1), DMA3_SLOT_B(2 * t + 1), DMA3_SLOT_B2(2 * t + 1))
            }
            DMA_WAIT();
            __syncthreads();
            if (kh + 1 == NKH && cb + 1 < NCB) {          // row 1 of the next channel block into the slot row 4 left
                row_burst(cb + 1, 1);
                DMA_WAIT();
                __syncthreads();
            }
#undef DMA3_TAP_C
#undef DMA3_TAP
#undef DMA3_ROW
#undef DMA3_NA
#undef DMA3_SLOT_A
#undef DMA3_NB
#undef DMA3_SLOT_B
#undef DMA3_SLOT_B2
        }
    }
    };
    if (!DMA3_SKIP) k_loop(std::integral_constant<int, -1>{});
    else if (c == 0) k_loop(std::integral_constant<int, 0>{});
    else k_loop(std::integral_constant<int, 1>{});
    conv_f16_epilogue<0>(acc, a, smem, b, h0, row, c, lane);
}

template <int T>
static int launch_f16_dma3(const ConvF16Args &a, int B, hipStream_t st)
{
    constexpr size_t lds = 2 * (2 * 7 * 2048) + 3 * (size_t)(4 * (CV_PITCH + 12 * T) / 64) * 1024;      // W[2] + three row slots
    static_assert(lds <= 160 * 1024, "LDS budget");
    static_assert(lds >= 96 * 1024, "the pooling epilogue's exchange area");
    static MxLdsLatch latch = {};                             // per device (common.h)
    if (mx_set_dyn_lds(latch, (const void *)conv_f16x3_dma3_kernel<T>, lds) != MX_OK) return MX_ERR_LAUNCH;
    hipLaunchKernelGGL((conv_f16x3_dma3_kernel<T>), dim3(a.H / 2, B), dim3(256), lds, st, a);
    return mx_launch_status();
}

template <int T>
static int launch_f16_dma16(const ConvF16Args &a, int B, hipStream_t st)
{
    constexpr int PWP = (CV_PITCH + 12 * T + 15) / 16 * 16;
    constexpr size_t lds = 2 * (2 * 7 * 2048) + 4 * (size_t)((4 * PWP + 63) / 64) * 1024;      // W[2] + four row slots
    static_assert(lds <= 160 * 1024, "LDS budget");
    static MxLdsLatch latch = {};                             // per device (common.h)
    if (mx_set_dyn_lds(latch, (const void *)conv_f16x3_dma16_kernel<T, true>, lds) != MX_OK) return MX_ERR_LAUNCH;
    hipLaunchKernelGGL((conv_f16x3_dma16_kernel<T, true>), dim3(a.H / 2, B), dim3(256), lds, st, a);
    return mx_launch_status();
}

template <int T>
static int launch_f16_dma(const ConvF16Args &a, int B, hipStream_t st)
{
    constexpr int PWP = CV_PITCH + 12 * T;
    constexpr size_t lds = 2 * (2 * 7 * 2048) + 2 * (size_t)((8 * PWP + 63) / 64) * 1024;
    static_assert(lds <= 160 * 1024, "LDS budget");
    static MxLdsLatch latch = {};                             // per device (common.h)
    if (mx_set_dyn_lds(latch, (const void *)conv_f16x3_dma_kernel<T>, lds) != MX_OK) return MX_ERR_LAUNCH;
    hipLaunchKernelGGL((conv_f16x3_dma_kernel<T>), dim3(a.H / 2, B), dim3(256), lds, st, a);
    return mx_launch_status();
}

template <int T, int OUTMODE>
static int launch_f16(const ConvF16Args &a, int B, hipStream_t st)
{
    constexpr int PWP = CV_PITCH + 12 * T;
    const size_t lds = (size_t)(2 * CV_KW * 64 * 16 + 2 * 2 * PWP * 16) * sizeof(_Float16);
    static MxLdsLatch latch = {};                             // per device (common.h)
    if (mx_set_dyn_lds(latch, (const void *)conv_f16x3_kernel<T, OUTMODE>, lds) != MX_OK) return MX_ERR_LAUNCH;
    hipLaunchKernelGGL((conv_f16x3_kernel<T, OUTMODE>), dim3(a.H / 2, B), dim3(256), lds, st, a);
    return mx_launch_status();
}

static int dispatch_f16(int T, int outmode, const ConvF16Args &a, int B, hipStream_t st)
{
    if (outmode == 0) {
        if (T == 1) return launch_f16_dma16<1>(a, B, st);
        if (T == 2) return launch_f16_dma16<2>(a, B, st);
        if (T == 4) return launch_f16_dma16<4>(a, B, st);
        if (T == 8) return launch_f16_dma3<8>(a, B, st);
        if (T == 16) return launch_f16_dma3<16>(a, B, st);
    } else {
        if (T == 1) return launch_f16_dma<1>(a, B, st);
        if (T == 2) return launch_f16_dma<2>(a, B, st);
        if (T == 4) return launch_f16_dma<4>(a, B, st);
        if (T == 8) return launch_f16<8, 1>(a, B, st);
        if (T == 16) return launch_f16<16, 1>(a, B, st);
    }
    return MX_ERR_UNSUPPORTED;
}

// ---- C ABI ------------------------------------------------------------------------------------------------
// weights (64,64,5,13) fp32 -> w_hi, w_lo: 4*5*13*64*16 halfs each (flip = 1 for the data gradient)
MX_EXPORT int mx_conv_pack_weights_f16(const float *W, int32_t flip, void *w_hi, void *w_lo, void *stream)
{
    if (!W || !w_hi || !w_lo) return MX_ERR_ARG;
    hipLaunchKernelGGL(pack_weights_f16_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, W, (int)flip,
                       (_Float16 *)w_hi, (_Float16 *)w_lo);
    return mx_launch_status();
}

// forward operand: x (B,64,H,352) previous block's pooled pre-activations, stats (B,64,2), slope (64,)
// -> x_hi, x_lo (B,H,4,352,16) fp16 = split of (prelu(x) - mean) * rstd
MX_EXPORT int mx_conv_prep_fwd_f16(const float *x, const float *stats, const float *slope, int64_t B, int64_t H,
                                   int64_t Wv, void *x_hi, void *x_lo, void *stream)
{
    if (!x || !stats || !slope || !x_hi || !x_lo || B <= 0 || H <= 0 || Wv <= 0 || Wv > CV_PITCH) return MX_ERR_ARG;
    if (B > 65535 || H > 65535) return MX_ERR_UNSUPPORTED;
    if (H % 4 == 0)
        hipLaunchKernelGGL((split_prep_fwd_kernel<4>), dim3(CV_PITCH / 32, (unsigned)(H / 4), (unsigned)B), dim3(256), 0,
                           (hipStream_t)stream, x, stats, slope, (int)H, (int)Wv, (_Float16 *)x_hi, (_Float16 *)x_lo);
    else
        hipLaunchKernelGGL((split_prep_fwd_kernel<1>), dim3(CV_PITCH / 32, (unsigned)H, (unsigned)B), dim3(256), 0,
                           (hipStream_t)stream, x, stats, slope, (int)H, (int)Wv, (_Float16 *)x_hi, (_Float16 *)x_lo);
    return mx_launch_status();
}

// dgrad operand: G, amax (B,64,H/2,352) -> dz_hi, dz_lo (B,H,4,352,16) fp16 = split of routed G * S_dz;
// scale (2,) device floats receives {S_dz, 1/S_dz} (S_dz = power of two from max|G|); amax_ws: 1 uint workspace,
// or -- amax_ready != 0 -- the bit pattern of max|G| that the producer of G already left there.
// dz_hi = dz_lo = NULL: only the scale pair is produced (the sparse kernels take the pooled operand of
// mx_conv_prep_gpool_cl_f16 instead of the routed one).
MX_EXPORT int mx_conv_prep_dgrad_f16(const float *G, const uint8_t *amax, int64_t B, int64_t H, int64_t Wv,
                                     uint32_t *amax_ws, int32_t amax_ready, float *scale, void *dz_hi, void *dz_lo,
                                     void *stream)
{
    if (!G || !amax || !amax_ws || !scale || B <= 0 || H < 2 || (H & 1) || Wv <= 0 || Wv > CV_PITCH) return MX_ERR_ARG;
    if ((dz_hi == nullptr) != (dz_lo == nullptr)) return MX_ERR_ARG;      // both NULL: only the scale pair is produced
    if (B > 65535 || H > 65535) return MX_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (!amax_ready) {          // otherwise *amax_ws already holds the bits of max|G| (mx_ln_prelu_bwd's gmax_bits)
        if (hipMemsetAsync(amax_ws, 0, sizeof(uint32_t), st) != hipSuccess) return MX_ERR_LAUNCH;
        const long long n4 = (long long)B * 64 * (H / 2) * CV_PITCH / 4;
        hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, st, G, n4, (int)Wv, amax_ws);
    }
    hipLaunchKernelGGL(pow2_scale_kernel, dim3(1), dim3(1), 0, st, amax_ws, scale);
    if (!dz_hi) return mx_launch_status();
    hipLaunchKernelGGL((split_prep_kernel<1>), dim3(CV_PITCH / 32, (unsigned)H, (unsigned)B), dim3(256), 0, st, G, amax,
                       nullptr, nullptr, scale, (int)H, (int)Wv, (_Float16 *)dz_hi, (_Float16 *)dz_lo);
    return mx_launch_status();
}

// forward conv (64 -> 64 channels, dilation in {1,2,4,8,16}) from prepared operands
MX_EXPORT int mx_conv_block_fwd_f16(const void *x_hi, const void *x_lo, const void *w_hi, const void *w_lo,
                                    const float *bias, int64_t B, int64_t H, int64_t Wv, int32_t dilation, float *out,
                                    uint8_t *out_amax, const float *slope_out, float *stats_part, void *stream)
{
    if (!x_hi || !x_lo || !w_hi || !w_lo || !bias || !out || !out_amax || (stats_part && !slope_out)) return MX_ERR_ARG;
    if (B <= 0 || B > 65535 || H < 2 || (H & 1) || Wv <= 0 || Wv > CV_PITCH) return MX_ERR_UNSUPPORTED;
    ConvF16Args a{(const _Float16 *)x_hi, (const _Float16 *)x_lo, (const _Float16 *)w_hi, (const _Float16 *)w_lo, bias,
                  nullptr, out, out_amax, (int)H, (int)Wv, slope_out, stats_part};
    return dispatch_f16(dilation, 0, a, (int)B, (hipStream_t)stream);
}

// data gradient from prepared operands (weights packed with flip = 1); scale = the {S_dz, 1/S_dz} pair
MX_EXPORT int mx_conv_block_dgrad_f16(const void *dz_hi, const void *dz_lo, const void *w_hi, const void *w_lo,
                                      const float *scale, int64_t B, int64_t H, int64_t Wv, int32_t dilation,
                                      float *dxhat, void *stream)
{
    if (!dz_hi || !dz_lo || !w_hi || !w_lo || !scale || !dxhat) return MX_ERR_ARG;
    if (B <= 0 || B > 65535 || H < 2 || (H & 1) || Wv <= 0 || Wv > CV_PITCH) return MX_ERR_UNSUPPORTED;
    ConvF16Args a{(const _Float16 *)dz_hi, (const _Float16 *)dz_lo, (const _Float16 *)w_hi, (const _Float16 *)w_lo,
                  nullptr, scale, dxhat, nullptr, (int)H, (int)Wv, nullptr, nullptr};
    return dispatch_f16(dilation, 1, a, (int)B, (hipStream_t)stream);
}

// ---- first block (2 input channels): one K stage (conv1_f16x3_tile_kernel) --------------------------------------
// W (64,2,5,13) -> w_hi, w_lo: 13*2*64*8 halfs each
MX_EXPORT int mx_conv_pack_weights_kvec_f16(const float *W, void *w_hi, void *w_lo, void *stream)
{
    if (!W || !w_hi || !w_lo) return MX_ERR_ARG;
    hipLaunchKernelGGL(pack_weights_kvec_f16_kernel, dim3(16), dim3(256), 0, (hipStream_t)stream, W, (_Float16 *)w_hi,
                       (_Float16 *)w_lo);
    return mx_launch_status();
}

// x (B,2,H,352) fp32 (log-mel), stats (B,2,2) -> xk_hi, xk_lo (B,H,352,16) fp16 = split of the LayerNorm-ed input,
// channel k = kh*2 + ci holding row h + kh - 2
MX_EXPORT int mx_conv_prep_fwd_kvec_f16(const float *x, const float *stats, int64_t B, int64_t H, int64_t Wv, void *xk_hi,
                                        void *xk_lo, void *stream)
{
    if (!x || !stats || !xk_hi || !xk_lo || B <= 0 || H <= 0 || Wv <= 0 || Wv > CV_PITCH) return MX_ERR_ARG;
    if (B > 65535 || H > 65535) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(split_prep_kvec_kernel, dim3((unsigned)((H + KV_ROWS - 1) / KV_ROWS), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, x, stats, (int)H, (int)Wv, (_Float16 *)xk_hi, (_Float16 *)xk_lo);
    return mx_launch_status();
}

// forward conv of the first block (2 -> 64 channels, dilation 1) + bias + max-pool from the k-vector operand
MX_EXPORT int mx_conv_block1_fwd_f16(const void *xk_hi, const void *xk_lo, const void *w_hi, const void *w_lo,
                                     const float *bias, int64_t B, int64_t H, int64_t Wv, float *out, uint8_t *out_amax,
                                     const float *slope_out, float *stats_part, void *stream)
{
    if (!xk_hi || !xk_lo || !w_hi || !w_lo || !bias || !out || !out_amax || (stats_part && !slope_out)) return MX_ERR_ARG;
    if (B <= 0 || B > 65535 || H < 2 || (H & 1) || Wv <= 0 || Wv > CV_PITCH) return MX_ERR_UNSUPPORTED;
    ConvF16Args a{(const _Float16 *)xk_hi, (const _Float16 *)xk_lo, (const _Float16 *)w_hi, (const _Float16 *)w_lo, bias,
                  nullptr, out, out_amax, (int)H, (int)Wv, slope_out, stats_part};
    // patch P[2] | 4 transposition images | sums | DMA descriptors (conv1_f16x3_tile_kernel)
    constexpr size_t lds = 2 * (size_t)((8 * (CV_PITCH + 12) + 63) / 64) * 1024 + 4 * 4352 + 8192 + 12 * 256 * sizeof(int);
    static_assert(lds <= 160 * 1024, "LDS budget");
    static MxLdsLatch latch_s = {}, latch_n = {};               // per device (common.h)
    if (mx_set_dyn_lds(latch_s, (const void *)conv1_f16x3_tile_kernel<true>, lds) != MX_OK ||
        mx_set_dyn_lds(latch_n, (const void *)conv1_f16x3_tile_kernel<false>, lds) != MX_OK)
        return MX_ERR_LAUNCH;
    const int n_tiles = (int)(B * (H / 2));
    int grid = 1024;                                            // 4 workgroups per CU over the launch: contiguous ranges, a short tail
    if (grid > n_tiles) grid = n_tiles;
    const int per = (n_tiles + grid - 1) / grid;
    grid = (n_tiles + per - 1) / per;
    if (stats_part) hipLaunchKernelGGL(conv1_f16x3_tile_kernel<true>, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, a, n_tiles, per);
    else hipLaunchKernelGGL(conv1_f16x3_tile_kernel<false>, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, a, n_tiles, per);
    return mx_launch_status();
}
