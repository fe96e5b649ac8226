// logmel_loss.hip -- log-mel L1 loss, value and gradient w.r.t. the prediction in one pass over the frames
// (reference: mod_extraction/losses.py:105-130 LogMelLoss: torchaudio MelSpectrogram(sr, n_fft, hop, n_mels) -- centre /
// reflect padding of n_fft/2, periodic Hann, power 2, HTK filter bank, no norm -- and
//   L = scale * mean |log max(M(y_hat), eps) - log max(M(y), eps)|  over rows x n_mels x frames, frames = 1 + T / hop).
//
// Gradient, torch's conventions (sgn(0) = 0; the clamp passes where M >= eps):
//   dM[m] = c sgn(la - lb) [M_a >= eps] / M_a  with c = scale / count,   dP[k] = sum_m fb[k, m] dM[m],   dL/dX[k] = 2 dP[k] X[k],
// then window, overlap-add by hop and the fold of the reflect padding.  c is known up front, so the time-domain gradient is
// complete once a frame's bins are: the pipeline of ola_ring.h (runs, frame pairs, ring, tails, fold) with a single gradient
// component.
//   lm_onepass : per frame: one forward transform of the prediction frame and one of the target frame (real input each: a packed
//                x + i y transform leaves the rounding of the louder frame on both spectra, and the log-domain gradient of a
//                weak band amplifies it) -> both powers P_a, P_b into the stream's exchange buffer -> the lanes take the mel
//                bands over their non-zero bin ranges (band_lo / band_hi, coefficients packed in LDS) -> |la - lb| into the
//                partial and dM into LDS -> each lane gathers dP of its bins over the (at most two, for a triangular bank)
//                bands that contain them -> gradient spectrum -> the pair's inverse transform and the ring.  Without dx: no
//                dM, no inverse transform, no ring.
//   finish     : value = scale * (sum of the fp64 per-workgroup partials, fixed order) / count
//   fold       : dx[n] (+)= the gradient at the padded positions that map to n
// Exact zeros: bit-identical (or negated) prediction and target frames go through the same arithmetic, so la == lb and the
// frame contributes 0 to the value and the gradient; an all-zero frame has power 0 exactly.
#include "ola_ring.h"

template <int N> struct LM {
    static constexpr int L = WF<N>::L, E = WF<N>::E, NB = WF<N>::NB, FW = WF<N>::FW;
    static constexpr int WAVES = (N == 2048) ? 2 : 4;          // wavefronts per workgroup
    static constexpr int STREAMS = WAVES * FW;                 // runs a workgroup works on
    static constexpr int NBIN = N / 2 / L;                     // bins per lane (plus the Nyquist bin on lane 0)
    static constexpr int NK = N / 2 + 1;                       // bins of the one-sided spectrum
};

// Dynamic LDS, in this order (each part a multiple of 8 bytes; rings first: ola_ring.h):  rings (STREAMS x N floats) |
// twiddles (N cf) | exchange buffers (STREAMS x LEN cf) | reduction (WAVES doubles) | dM (STREAMS x n_mels floats) |
// packed coefficients (coef_cap floats) | boff (n_mels + 1 ints) | band_lo (n_mels ints) | band range of every bin: lo, hi
// (2 x NK ints)
__host__ __device__ __forceinline__ size_t lm_align8(size_t v) { return (v + 7) & ~(size_t)7; }
template <int N> static size_t lm_lds_bytes(int n_mels, int coef_cap)
{
    using K = LM<N>;
    return (size_t)K::STREAMS * N * 4 + (size_t)N * 8 + (size_t)K::STREAMS * WF<N>::LEN * 8 + K::WAVES * 8 +
           lm_align8((size_t)K::STREAMS * n_mels * 4) + lm_align8((size_t)coef_cap * 4) + lm_align8((size_t)(2 * n_mels + 1) * 4) +
           lm_align8((size_t)2 * K::NK * 4);
}

template <int N, bool GRAD>
__global__ __launch_bounds__(LM<N>::WAVES * 64) void lm_onepass_kernel(
    const float *__restrict__ x, long long xs, const float *__restrict__ y, long long ys, const float *__restrict__ win,
    const float2 *__restrict__ tw, const float *__restrict__ fb, const int *__restrict__ band_lo, const int *__restrict__ band_hi,
    int n_mels, int coef_cap, int T, int hop, OlaRuns rg, float eps, float c, double *__restrict__ part,
    float *__restrict__ mainp, float *__restrict__ tails)
{
    using K = LM<N>;
    constexpr int L = K::L, E = K::E, NB = K::NB, FW = K::FW, STREAMS = K::STREAMS, NBIN = K::NBIN, NK = K::NK, NT = K::WAVES * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_smem[];
    size_t off = 0;
    float *rings = reinterpret_cast<float *>(lm_smem);
    off += (size_t)STREAMS * N * 4;
    cf *tw_s = reinterpret_cast<cf *>(lm_smem + off);
    off += (size_t)N * 8;
    cf *xbuf = reinterpret_cast<cf *>(lm_smem + off);
    off += (size_t)STREAMS * WF<N>::LEN * 8;
    double *red = reinterpret_cast<double *>(lm_smem + off);
    off += K::WAVES * 8;
    float *dm_all = reinterpret_cast<float *>(lm_smem + off);
    off += lm_align8((size_t)STREAMS * n_mels * 4);
    float *coef = reinterpret_cast<float *>(lm_smem + off);
    off += lm_align8((size_t)coef_cap * 4);
    int *boff = reinterpret_cast<int *>(lm_smem + off);
    int *blo = boff + n_mels + 1;
    off += lm_align8((size_t)(2 * n_mels + 1) * 4);
    int *kbl = reinterpret_cast<int *>(lm_smem + off), *kbh = kbl + NK;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane / L, a_ = lane % L;
    const int b = blockIdx.y, sidx = wave * FW + g;
    const int n_frames = rg.n_frames, F = rg.F;
    const float *xb = x + (size_t)b * xs, *yb = y + (size_t)b * ys;
    cf *buf = xbuf + (size_t)sidx * WF<N>::LEN;
    float *pw = reinterpret_cast<float *>(buf);                   // P_a[k] at k, P_b[k] at NK + k (2 NK <= 2 LEN floats)
    float *dm = dm_all + (size_t)sidx * n_mels;

    // ---- per workgroup: twiddles, band tables (ranges clamped to the spectrum), packed coefficients, the band range of every bin
    stage_twiddles<N, 1, NT>(tw_s, tw);
    for (int k = tid; k < NK; k += NT) { kbl[k] = n_mels; kbh[k] = 0; }
    if (GRAD)
        for (int j = a_; j < N; j += L) rings[(size_t)sidx * N + j] = 0.0f;
    // boff = exclusive prefix sum of the band widths: a contiguous chunk of bands per thread, a workgroup scan of the chunk
    // sums (a serial loop over the bands on one thread: 75 -> 68 us for a 128 x 1024 chunk, value + gradient)
    __shared__ int wsum[K::WAVES];
    {
        const int per = (n_mels + NT - 1) / NT, m0 = min(tid * per, n_mels), m1 = min(m0 + per, n_mels);
        int s = 0;
        for (int m = m0; m < m1; ++m) {
            const int lo = max(band_lo[m], 0), hi = min(band_hi[m], NK), w = hi > lo ? hi - lo : 0;
            blo[m] = lo;
            boff[m] = w;
            s += w;
        }
        int v = s;                                                // inclusive scan over the wavefront
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int ex = v - s;
        for (int w = 0; w < wave; ++w) ex += wsum[w];
        for (int m = m0; m < m1; ++m) {
            const int w = boff[m];
            boff[m] = ex;
            ex += w;
        }
        if (tid == NT - 1) boff[n_mels] = ex;
    }
    __syncthreads();
    const bool packed = boff[n_mels] <= coef_cap;                 // workgroup-uniform; otherwise the bands read fb directly
    for (int m = tid; m < n_mels; m += NT) {
        const int lo = blo[m], hi = lo + boff[m + 1] - boff[m], o = boff[m];
        for (int kk = lo; kk < hi; ++kk) {
            if (packed) coef[o + kk - lo] = fb[(size_t)kk * n_mels + m];
            if (GRAD) {
                atomicMin(&kbl[kk], m);                           // integer LDS atomics: the result is order-independent
                atomicMax(&kbh[kk], m + 1);
            }
        }
    }
    __syncthreads();
    // fb[k, m] for lo[m] <= k < hi[m]
    auto fbv = [&](int k, int m) -> float {
        if (!packed) return fb[(size_t)k * n_mels + m];
        const int lo = blo[m];
        return (k >= lo && k < lo + boff[m + 1] - boff[m]) ? coef[boff[m] + k - lo] : 0.0f;
    };

    FftLane<N> fl;
    fft_lane_setup<N, 1>(fl, buf, tw_s, tw, a_);
    const int run = blockIdx.x * STREAMS + sidx;
    const int f_begin = run * F, f_end = min(f_begin + F, n_frames);          // (an idle stream: f_begin >= f_end)
    float wv[E];                                                              // the lane's window values: positions a + L m
#pragma unroll
    for (int m = 0; m < E; ++m) wv[m] = win[a_ + L * m];
    double s_l[1] = {0.0};
    int base = 0;                                                             // ring slot of the current frame's position 0
    const unsigned ring_b = (unsigned)sidx * 4u * N;
    float *mb = GRAD ? mainp + (size_t)b * n_frames * hop : nullptr;

    cf raw[NB][4];                                                            // the next frame's unwindowed samples
    prefetch_frame<N>(raw, xb, yb, f_begin, f_end, n_frames, hop, T, a_);
    for (int fp = 0; fp < F; fp += 2) {
        int a = a_;
        asm volatile("" : "+v"(a));                                           // see mr_onepass_kernel
        const int f0 = f_begin + fp, f1 = f0 + 1;
        if (__ballot(f0 < f_end) == 0ull) break;                               // every stream of the wavefront is done
        const bool live0 = f0 < f_end, live1 = f1 < f_end;
        cf ga[NBIN];                                                           // G~ of frame f0 at the lane's bins
        float nya = 0.0f, nyb = 0.0f;                                          // ... and of both frames at the Nyquist bin (real; lane 0)
        cf R[NB][4], Z[E];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool live = u ? live1 : live0;
            // prediction, then target: ONE real frame per transform, so that each spectrum carries the rounding of its own
            // level only (a packed x + i y transform measured 2-3x the fp32 yardstick's gradient error on weak bands), the
            // two spectra of bit-identical (or negated) frames come out bit-identical (negated), and an all-zero frame has
            // an all-zero spectrum
            cf Xs[NBIN];                                                       // X[k] of the lane's bins
            float pa[NBIN], pb[NBIN], xny = 0.0f, pany = 0.0f, pbny = 0.0f;
#pragma unroll
            for (int sg = 0; sg < 2; ++sg) {
#pragma unroll
                for (int bq = 0; bq < NB; ++bq)
#pragma unroll
                    for (int cq = 0; cq < 4; ++cq)
                        R[bq][cq] = cf{(sg ? raw[bq][cq].y : raw[bq][cq].x) * wv[m_of_in<N>(bq, cq)], 0.0f};
                if (sg) prefetch_frame<N>(raw, xb, yb, u ? f0 + 2 : f1, f_end, n_frames, hop, T, a);     // in flight during this transform
                wave_fft<N, false>(R, Z, fl);
#pragma unroll
                for (int i = 0; i < E; ++i) buf[pos_final<N>(i, a)] = Z[i];
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int j = 0; j < NBIN; ++j) {
                    const cf z = buf[a + L * j];
                    const float p = __builtin_fmaf(z.x, z.x, z.y * z.y);
                    if (sg) pb[j] = p;
                    else { Xs[j] = z; pa[j] = p; }
                }
                if (a == 0) {                                                  // Nyquist bin
                    const cf z = buf[N / 2];
                    const float p = __builtin_fmaf(z.x, z.x, z.y * z.y);
                    if (sg) pbny = p;
                    else { xny = z.x; pany = p; }
                }
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
            for (int j = 0; j < NBIN; ++j) {
                pw[a + L * j] = pa[j];
                pw[NK + a + L * j] = pb[j];
            }
            if (a == 0) { pw[N / 2] = pany; pw[NK + N / 2] = pbny; }
            __builtin_amdgcn_wave_barrier();
            // mel bands of the lane: m = a + L i, over their non-zero bins (the forward's order: one fmaf per bin, ascending)
            float fsum = 0.0f;
            for (int m = a; m < n_mels; m += L) {
                float ma = 0.0f, mb_ = 0.0f;
                const int lo = blo[m], hi = lo + boff[m + 1] - boff[m];
                if (packed) {
                    const float *cm = coef + boff[m] - lo;
                    for (int kk = lo; kk < hi; ++kk) {
                        ma = __builtin_fmaf(cm[kk], pw[kk], ma);
                        mb_ = __builtin_fmaf(cm[kk], pw[NK + kk], mb_);
                    }
                } else {
                    for (int kk = lo; kk < hi; ++kk) {
                        const float w = fb[(size_t)kk * n_mels + m];
                        ma = __builtin_fmaf(w, pw[kk], ma);
                        mb_ = __builtin_fmaf(w, pw[NK + kk], mb_);
                    }
                }
                const float dl = __builtin_amdgcn_logf(fmaxf(ma, eps)) - __builtin_amdgcn_logf(fmaxf(mb_, eps));   // log2
                fsum += fabsf(dl);
                if (GRAD) {
                    const float sg = dl > 0.0f ? c : (dl < 0.0f ? -c : 0.0f);
                    dm[m] = (live && ma >= eps) ? sg / ma : 0.0f;
                }
            }
            if (live) s_l[0] += (double)(0.69314718055994531f * fsum);
            if (GRAD) {
                __builtin_amdgcn_wave_barrier();
                // dP of the lane's bins over the bands that contain them; G~[k] = dP X (= G / 2, the Hermitian completion's
                // share; DC and Nyquist: G = 2 dP X itself)
                auto dpk = [&](int k) {
                    float s = 0.0f;
                    const int m1 = kbh[k];
                    for (int m = kbl[k]; m < m1; ++m) s = __builtin_fmaf(fbv(k, m), dm[m], s);
                    return s;
                };
#pragma unroll
                for (int j = 0; j < NBIN; ++j) {
                    const int k = a + L * j;
                    const bool dc = (j == 0) && (a == 0);
                    const float dp = dpk(k);
                    const cf gk = Xs[j] * (dc ? 2.0f * dp : dp);
                    if (u == 0) ga[j] = gk;
                    else place_pair<N>(R, buf, j, a, pair_h(dc, ga[j], gk), mirror_h(ga[j], gk));
                }
                if (a == 0) {
                    const float nv = 2.0f * dpk(N / 2) * xny;
                    if (u == 0) nya = nv;
                    else nyb = nv;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (GRAD) {
            pair_finish<N>(R, buf, a, nya, nyb);
            wave_fft<N, true>(R, Z, fl);
            asm volatile("" : "+v"(a));
            ring_add_and_flush<N>(lm_smem, ring_b, mb, Z, wv, f0, live0, live1, a, base, hop);
            base = (base + 2 * hop) & (N - 1);
        }
    }
    if (GRAD && f_begin < f_end) ring_write_tail<N, 1>(rings + (size_t)sidx * N, tails, rg, b, run, f_end - f_begin, hop, a_);
    block_partials<1, K::WAVES>(s_l, red, b, part);
}

// partial sums -> value = scale * mean |la - lb|
__global__ __launch_bounds__(256) void lm_finish_kernel(const double *__restrict__ part, int n_part, double scale_over_count,
                                                        float *__restrict__ value)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256) s += part[i];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) value[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * scale_over_count);
}

__global__ __launch_bounds__(256) void lm_fold_kernel(OlaGrad r, int T, int accumulate, float *__restrict__ dx, long long ds)
{
    const int b = blockIdx.y, B = gridDim.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= T) return;
    float acc = 0.0f;
    for_padded_positions(n, r.N, T, [&](int p) {
        float g[1] = {0.0f};
        fold_pos<1>(r, B, b, p, g);
        acc += g[0];
    });
    float *o = dx + (size_t)b * ds + n;
    *o = accumulate ? *o + acc : acc;
}

template <int N>
static int lm_run(const float *x, long long xs, const float *y, long long ys, const float *win, const float2 *tw, const float *fb,
                  const int *band_lo, const int *band_hi, int n_mels, int B, int T, int hop, float eps, float scale, int accumulate,
                  double *part, float *scratch, float *value, float *dx, long long ds, hipStream_t st)
{
    using K = LM<N>;
    const OlaRuns rg = ola_runs(N, hop, T);
    const int groups = (rg.n_runs + K::STREAMS - 1) / K::STREAMS;
    const int coef_cap = 2 * K::NK + 2 * n_mels;                  // triangular filters: every bin lies in <= 2 bands
    const size_t lds = lm_lds_bytes<N>(n_mels, coef_cap);
    const size_t lds_cap = 160 * 1024 - 64;                       // (the kernel's static LDS: the scan's wave sums)
    if (lds > lds_cap) return MX_ERR_UNSUPPORTED;
    const long long count = (long long)B * n_mels * rg.n_frames;
    const float c = (float)((double)scale / (double)count);
    float *mainp = scratch, *tails = dx ? scratch + ola_main_floats(B, rg, hop) : nullptr;
    static MxLdsLatch latch[2];
    const void *fn = dx ? (const void *)lm_onepass_kernel<N, true> : (const void *)lm_onepass_kernel<N, false>;
    if (lds > 64 * 1024 && mx_set_dyn_lds(latch[dx ? 1 : 0], fn, lds_cap) != MX_OK) return MX_ERR_LAUNCH;
    if (dx)
        hipLaunchKernelGGL((lm_onepass_kernel<N, true>), dim3(groups, B), dim3(K::WAVES * 64), lds, st, x, xs, y, ys, win, tw, fb,
                           band_lo, band_hi, n_mels, coef_cap, T, hop, rg, eps, c, part, mainp, tails);
    else
        hipLaunchKernelGGL((lm_onepass_kernel<N, false>), dim3(groups, B), dim3(K::WAVES * 64), lds, st, x, xs, y, ys, win, tw, fb,
                           band_lo, band_hi, n_mels, coef_cap, T, hop, rg, eps, c, part, nullptr, nullptr);
    hipLaunchKernelGGL(lm_finish_kernel, dim3(1), dim3(256), 0, st, part, groups * B, (double)scale / (double)count, value);
    if (dx)
        hipLaunchKernelGGL(lm_fold_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, st,
                           OlaGrad{mainp, tails, N, hop, rg}, T, accumulate, dx, ds);
    return mx_launch_status();
}

// See include/modex_hip.h.
MX_EXPORT int mx_logmel_l1_loss(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B, int64_t T,
                                const float *window, const float *twiddle, const float *fb, const int32_t *band_lo,
                                const int32_t *band_hi, int64_t n_fft, int64_t hop, int64_t n_mels, float eps, float scale,
                                int32_t accumulate, double *part, float *scratch, float *value, float *dx, int64_t dx_stride,
                                void *stream)
{
    if (!y_hat || !y || !window || !twiddle || !fb || !band_lo || !band_hi || !part || !value || (dx && !scratch) || B <= 0 ||
        T <= 0 || hop <= 0 || n_mels <= 0 || !(eps > 0.0f))
        return MX_ERR_ARG;
    if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return MX_ERR_UNSUPPORTED;
    if (T <= n_fft / 2) return MX_ERR_ARG;                        // the reflect padding needs more than n_fft / 2 samples
    if (B > 65535 || T >= (1ll << 30) || n_mels > 2048 || (long long)(1 + T / hop) * hop >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
#define LM_CALL(NN)                                                                                                                \
    lm_run<NN>(y_hat, (long long)y_hat_stride, y, (long long)y_stride, window, (const float2 *)twiddle, fb, band_lo, band_hi,       \
               (int)n_mels, (int)B, (int)T, (int)hop, eps, scale, accumulate, part, scratch, value, dx, (long long)dx_stride, st)
    if (n_fft == 512) return LM_CALL(512);
    if (n_fft == 1024) return LM_CALL(1024);
    return LM_CALL(2048);
#undef LM_CALL
}
