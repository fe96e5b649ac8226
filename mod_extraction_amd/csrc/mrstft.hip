// mrstft.hip -- K11: multi-resolution STFT loss, forward value and gradient w.r.t. the prediction
// (reference: mod_extraction/losses.py:155-156 -> auraloss==0.4.0 MultiResolutionSTFTLoss(reduction=
// "mean"); third-party, source absent from the reference tree: PARITY UNPINNED, checked against
// oracle/losses.py:MultiResolutionSTFTLoss, which restates the published auraloss defaults:
// (n_fft, hop, win) = (1024,120,600), (2048,240,1200), (512,50,240), periodic hann centred in the FFT
// frame, centre=True reflect padding, mag = sqrt(clamp(re^2 + im^2, eps)),
// loss = mean over resolutions of [ ||Y - X||_F / ||Y||_F  +  mean |log X - log Y| ]).
//
// Value + gradient: ONE pass over the frames per resolution, no per-bin workspace (12 B/sample algorithmic: x, y in, grad out).
//   dL/dX of a bin = alpha_r * G1 + G2 with  G1 = (|X| - |Y|) X / |X|,  G2 = c_log sign(log|X| - log|Y|) / |X| * X / |X|,
//   c_log = w_log / (n_res * count) known up front and alpha_r = w_sc / (n_res ||Y - X||_F ||Y||_F) the ONLY global quantity --
//   a scalar multiplier.  Window, inverse transform, overlap-add and the reflect-padding fold are linear, so the kernel
//   that holds a frame's bins carries G1 and G2 to the time domain separately and a small last pass forms
//   alpha_r g1_r + g2_r:  nothing per bin is written to memory (the two-pass version parked 12 B per bin and re-read
//   them once the norms were known: 25 GB per 256 x 4 s step, 46x the algorithmic bytes).
//   onepass : the pipeline of ola_ring.h (runs, frame pairs, rings, tails) with two gradient components.  Per frame: forward
//             FFT of x + i*s*y (register-staged radix-4 Stockham, wave_fft.h) -> both spectra by Hermitian separation -> loss
//             sums and the frame's G1, G2; the pair's G1 spectra go through one inverse FFT, likewise G2: two transforms
//             per frame (it was 1.5, plus 24 B per bin of traffic), two rings per stream.
//   finish  : loss terms and alpha_r from the per-workgroup partial sums
//   fold    : dx[n] = sum_r sum_{padded positions p of n} ( alpha_r g1_r[p] + g2_r[p] )
// Value only (dx == NULL): pass A (mr_stats_kernel) + finish.
// Packing (both forward kernels): the Hermitian split leaves an error of about u ||louder windowed frame|| on BOTH spectra, so
// each frame's target is scaled by s = 2^k, k = round(log2(||x_w|| / ||y_w||)) clamped to +-60 (0 for an all-zero frame and
// for |k| < 2), to the prediction's level before packing, and |Y|^2 = |D|^2 s^-2 exactly (pack_gain).  The gradient transforms
// carry X only.
// Frames whose windowed x and y are bit-identical or bit-negated take |Y| := |X| (frame_same, on the unscaled frames).
// Measured per 256 clips x 4 s (all three resolutions, value + gradient): 19.2 ms (frame spread over 256 threads, an LDS
// round trip and a __syncthreads per pass, twiddles from global memory) -> 14.9 (twiddles staged in LDS) -> 11.4 ms (one frame
// per wavefront) -> 7.0 ms (parked bins, paired inverse, hardware transcendentals, LDS spans) -> this file.
// The FFT passes are VALU-issue bound.
#include "ola_ring.h"

#define MR_FPG 16        // frames per workgroup (value-only pass); the partial-sum workspace is sized for >= 8
#define MR_OPW 4         // wavefronts per workgroup of the one-pass kernel
#ifndef MR_OP_EU
#define MR_OP_EU 2       // waves per SIMD the 512 / 1024 one-pass kernels are compiled for (2048: 1, its LDS leaves one workgroup per CU)
#endif

// frame f of x + i*y, windowed, centre / reflect padded, straight into the stage-A register layout.  INTERIOR (wave-uniform):
// the frame does not touch either end of the clip, so no position needs the reflection arithmetic (two compares and selects per
// load) and the loads are one base pointer + constant offsets; all but the first and last N / (2 hop) frames of a clip.
template <int N, bool INTERIOR>
__device__ __forceinline__ void load_frame(cf (&R)[WF<N>::NB][4], const float *xb, const float *yb, const float *win,
                                           int f, int hop, int T, int a)
{
    const float *xf = xb + (f * hop - N / 2 + a), *yf = yb + (f * hop - N / 2 + a);     // dereferenced only when INTERIOR
#pragma unroll
    for (int b = 0; b < WF<N>::NB; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = a + WF<N>::L * b + (N / 4) * c;
            const float w = win[n];
            if (INTERIOR) {
                R[b][c] = {xf[WF<N>::L * b + (N / 4) * c] * w, yf[WF<N>::L * b + (N / 4) * c] * w};
            } else {
                const int s = reflect_index(f * hop + n - N / 2, T);
                R[b][c] = {xb[s] * w, yb[s] * w};
            }
        }
}

// spectra of the two real signals from Z = FFT(x + i y):  X[k] = (Z[k] + conj Z[N-k]) / 2,
// Y[k] = (Z[k] - conj Z[N-k]) / (2 i)
template <int N>
__device__ __forceinline__ void split_bins(const cf *Z, int k, cf &X, cf &Y)
{
    const cf z = Z[k], zc = Z[(N - k) & (N - 1)];
    X = {0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y)};
    Y = {0.5f * (z.y + zc.y), -0.5f * (z.x - zc.x)};
}

// the lane's frame slot of iteration `it`: frame index within the workgroup's MR_FPG frames
template <int N> __device__ __forceinline__ int frame_slot(int it, int wave, int g)
{
    return (it * WF<N>::WAVES + wave) * WF<N>::FW + g;
}

// ---- pass A -------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(WF<N>::WAVES * 64) __attribute__((amdgpu_waves_per_eu(2))) void mr_stats_kernel(const float *__restrict__ x, long long xs,
                                                                     const float *__restrict__ y, long long ys,
                                                                     const float *__restrict__ win,
                                                                     const float2 *__restrict__ tw, int T, int hop,
                                                                     int n_frames, float eps,
                                                                     double *__restrict__ part)
{
    constexpr int L = WF<N>::L, E = WF<N>::E, WAVES = WF<N>::WAVES, FW = WF<N>::FW;
    __shared__ cf xbuf[WAVES * FW][WF<N>::LEN];
    __shared__ cf tw_s[N];
    __shared__ double red[WAVES * 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / L, a_ = lane % L;
    const int b = blockIdx.y;
    const float *xb = x + (size_t)b * xs, *yb = y + (size_t)b * ys;
    cf *buf = xbuf[wave * FW + g];
    stage_twiddles<N, MR_MAXN / N, WAVES * 64>(tw_s, tw);
    __syncthreads();
    FftLane<N> fl;
    fft_lane_setup<N>(fl, buf, tw_s, tw, a_);
    double s[3] = {0.0, 0.0, 0.0};                                       // sum d^2, sum Ym^2, sum |log Xm - log Ym|
    for (int it = 0; it < MR_FPG / (WAVES * FW); ++it) {
        int a = a_;                                                      // opaque per iteration: see mr_onepass_kernel
        asm volatile("" : "+v"(a));
        const int f = blockIdx.x * MR_FPG + frame_slot<N>(it, wave, g);
        if (f - g >= n_frames) break;                                   // wave-uniform (frames of a wave are f-g, f-g+1)
        const bool live = f < n_frames;
        cf R[WF<N>::NB][4], Z[E];
        {
            // frames of this wave: f - g (and f - g + 1 for the two-frame layout of 512)
            const int fa = f - g, fz = fa + FW - 1;
            const bool interior = fa * hop - N / 2 >= 0 && fz * hop + N / 2 <= T && fz < n_frames;     // wave-uniform
            if (interior) load_frame<N, true>(R, xb, yb, win, f, hop, T, a);
            else load_frame<N, false>(R, xb, yb, win, live ? f : n_frames - 1, hop, T, a);
        }
        const cf e = frame_energy<N>(R);
        const bool same = frame_same<N>(R, g, e);
        const float sinv2 = pack_gain<N>(R, same, e);
        wave_fft<N, false>(R, Z, fl);
#pragma unroll
        for (int i = 0; i < E; ++i) buf[pos_final<N>(i, a)] = Z[i];
        __builtin_amdgcn_wave_barrier();
        if (live) {
            // Bin pass.  Hardware square root / log2 (1 ulp; the library versions' range fix-ups were 40 % of this kernel's
            // instructions), log Xm - log Ym = ln2 / 2 * (log2 max(|X|^2, eps) - log2 max(|Y|^2, eps)), Ym^2 = max(|Y|^2, eps),
            // and the frame's <= 9 terms per lane summed in fp32 before they enter the fp64 accumulators.
            float fd = 0.0f, fy = 0.0f, fl = 0.0f;
            auto bin = [&](int k) {
                cf X, Y;
                split_bins<N>(buf, k, X, Y);
                const float px = X.x * X.x + X.y * X.y;
                const float cx = fmaxf(px, eps), cy = fmaxf(same ? px : (Y.x * Y.x + Y.y * Y.y) * sinv2, eps);
                const float d = __builtin_amdgcn_sqrtf(cy) - __builtin_amdgcn_sqrtf(cx);
                fd += d * d;
                fy += cy;
                fl += fabsf(__builtin_amdgcn_logf(cx) - __builtin_amdgcn_logf(cy));
            };
#pragma unroll
            for (int j = 0; j < N / 2 / L; ++j) bin(a + L * j);
            if (a == 0) bin(N / 2);
            s[0] += (double)fd;
            s[1] += (double)fy;
            s[2] += (double)(0.5f * 0.69314718055994531f * fl);
        }
        __builtin_amdgcn_wave_barrier();
    }
    block_partials<3, WAVES>(s, red, b, part);
}

// partial sums of one resolution -> terms[0] = sc, terms[1] = log-mag; coef (2,) for pass B
__global__ __launch_bounds__(256) void mr_finish_kernel(const double *__restrict__ part, int n_part, long long count,
                                                        float w_sc, float w_log, float res_scale,
                                                        float *__restrict__ terms, float *__restrict__ coef)
{
    __shared__ double red[4][3];
    double s_d = 0.0, s_y = 0.0, s_l = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256) { s_d += part[i * 3]; s_y += part[i * 3 + 1]; s_l += part[i * 3 + 2]; }
    s_d = wave_sum_f64(s_d); s_y = wave_sum_f64(s_y); s_l = wave_sum_f64(s_l);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = s_d; red[wave][1] = s_y; red[wave][2] = s_l; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    s_d = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    s_y = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    s_l = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    const double nd = sqrt(s_d), ny = sqrt(s_y);
    terms[0] = (float)(nd / ny);
    terms[1] = (float)(s_l / (double)count);
    // d sc / d Xm = (Xm - Ym) / (||Y-X|| * ||Y||): the scalar alpha of this resolution (0 for identical signals: the exact-zero
    // gradient of the reference's 0 / 0-free path); d logmag / d Xm = sign(log Xm - log Ym) / (count * Xm) went into G2 already
    coef[0] = nd > 0.0 ? (float)((double)res_scale * w_sc / (nd * ny)) : 0.0f;
}

// ---- the one-pass value + gradient kernel ------------------------------------------------------------------------
// One bin of one frame.  Works on the DOUBLED spectra straight from the Hermitian separation of Z = FFT(x + i y),
//   X2 = Z[k] + conj Z[N-k] = 2 X,   D = Z[k] - conj Z[N-k]  with |D| = 2 |Y|  (only |Y| enters the loss),
// two packed adds; every constant factor is folded into the scalars: the three loss sums come out 4x (d^2, Ym^2) or unscaled
// (the log difference) and are rescaled once per frame, and the function returns s1', s2' such that s' X2 = G / 2 -- the
// Hermitian-completed gradient spectrum G~[k] = G[k] / 2 the inverse transform wants (DC and Nyquist: G itself = 2 s' X2).
// With G1 = (Xm - Ym) X / Xm and G2 = c_log sign(log Xm - log Ym) X / Xm^2:  s1' = (Xm2 - Ym2) / (4 Xm2),  s2' = +-c_log / Xm2^2
// (Xm2 = 2 Xm).  Branch-free; hardware square root / reciprocal / log2 (1 ulp each, no range fix-ups: the library sqrtf, two logf
// and two divisions were 70 of ~90 instructions per bin); Xm and Ym by the same formula, so that X == Y gives exactly 0; the clamp
// passes no gradient below eps.
struct BinOut { float s1, s2; };
// D comes from the level-equalised pack (pack_gain): |D|^2 sinv2 is the target's, exactly.
__device__ __forceinline__ BinOut bin_terms(const cf &X2, const cf &D, bool same, float sinv2, float eps4, float c_log, float &fd,
                                            float &fy, float &fl)
{
    const float px = __builtin_fmaf(X2.x, X2.x, X2.y * X2.y);
    const float py = same ? px : __builtin_fmaf(D.x, D.x, D.y * D.y) * sinv2;
    const float cx = fmaxf(px, eps4), cy = fmaxf(py, eps4);
    const float xm = __builtin_amdgcn_sqrtf(cx), ym = __builtin_amdgcn_sqrtf(cy);
    const float d = xm - ym;
    const float dl = __builtin_amdgcn_logf(cx) - __builtin_amdgcn_logf(cy);       // 2 / ln 2 * (log Xm - log Ym)
    fd = __builtin_fmaf(d, d, fd);
    fy += cy;
    fl += fabsf(dl);
    const float rx = __builtin_amdgcn_rcpf(xm);
    const float sg = dl > 0.0f ? c_log : (dl < 0.0f ? -c_log : 0.0f);
    const bool pass = px > eps4;
    return {pass ? 0.25f * d * rx : 0.0f, pass ? sg * rx * rx : 0.0f};
}

template <int N> struct OP {
    static constexpr int L = WF<N>::L, E = WF<N>::E, NB = WF<N>::NB, FW = WF<N>::FW;
    static constexpr int STREAMS = MR_OPW * FW;                  // runs a workgroup works on
    static constexpr int NBIN = N / 2 / L;                      // bins per lane (plus the Nyquist bin on lane 0): 8, 8, 16
    static constexpr size_t lds_bytes() { return (size_t)N * 8 + (size_t)STREAMS * WF<N>::LEN * 8 + (size_t)STREAMS * 2 * N * 4 + MR_OPW * 3 * 8; }
};

template <int N>
__global__ __launch_bounds__(MR_OPW * 64) __attribute__((amdgpu_waves_per_eu(N == 2048 ? 1 : MR_OP_EU))) void mr_onepass_kernel(
    const float *__restrict__ x, long long xs, const float *__restrict__ y, long long ys, const float *__restrict__ win,
    const float2 *__restrict__ tw, int T, int hop, OlaRuns rg, float eps, float c_log,
    double *__restrict__ part, float *__restrict__ main1, float *__restrict__ main2, float *__restrict__ tails)
{
    constexpr int L = OP<N>::L, E = OP<N>::E, NB = OP<N>::NB, FW = OP<N>::FW, STREAMS = OP<N>::STREAMS, NBIN = OP<N>::NBIN;
    extern __shared__ __attribute__((aligned(16))) unsigned char op_smem[];
    // rings first (ola_ring.h): ring c of stream s starts at byte (2 s + c) 4 N
    float *rings = reinterpret_cast<float *>(op_smem);
    cf *tw_s = reinterpret_cast<cf *>(op_smem + (size_t)STREAMS * 2 * N * 4);
    cf *xbuf = reinterpret_cast<cf *>(op_smem + (size_t)STREAMS * 2 * N * 4 + (size_t)N * 8);
    double *red = reinterpret_cast<double *>(op_smem + (size_t)N * 8 + (size_t)STREAMS * WF<N>::LEN * 8 + (size_t)STREAMS * 2 * N * 4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / L, a_ = lane % L;
    const int b = blockIdx.y, sidx = wave * FW + g;
    const int n_frames = rg.n_frames, F = rg.F;
    const float *xb = x + (size_t)b * xs, *yb = y + (size_t)b * ys;
    cf *buf = xbuf + (size_t)sidx * WF<N>::LEN;
    float *ring1 = rings + (size_t)sidx * 2 * N;
    stage_twiddles<N, MR_MAXN / N, MR_OPW * 64>(tw_s, tw);
    for (int j = a_; j < 2 * N; j += L) ring1[j] = 0.0f;
    __syncthreads();
    FftLane<N> fl;
    fft_lane_setup<N>(fl, buf, tw_s, tw, a_);

    const int run = blockIdx.x * STREAMS + sidx;
    const int f_begin = run * F, f_end = min(f_begin + F, n_frames);          // (an idle stream: f_begin >= f_end)
    float wv[E];                                                              // the lane's window values: positions a + L m
#pragma unroll
    for (int m = 0; m < E; ++m) wv[m] = win[a_ + L * m];
    double s[3] = {0.0, 0.0, 0.0};                                            // sum d^2, sum Ym^2, sum |log Xm - log Ym|
    int base = 0;                                                             // ring slot of the current frame's position 0
    const unsigned ring1_b = (unsigned)(sidx * 2) * 4u * N, ring2_b = ring1_b + 4u * N;
    float *m1 = main1 + (size_t)b * n_frames * hop, *m2 = main2 + (size_t)b * n_frames * hop;

    cf raw[NB][4];                                                            // the next frame's unwindowed samples
    prefetch_frame<N>(raw, xb, yb, f_begin, f_end, n_frames, hop, T, a_);
    for (int fp = 0; fp < F; fp += 2) {
        // the lane's position is made opaque to the optimiser again before every transform: the ~100 twiddle / exchange /
        // window addresses built from it would otherwise be shared by the iteration's four transforms (and hoisted out of the
        // frame loop) and live in scratch memory (21 / 30 spilled registers for N = 1024 / 2048)
        int a = a_;
        asm volatile("" : "+v"(a));
        const int f0 = f_begin + fp, f1 = f0 + 1;
        if (__ballot(f0 < f_end) == 0ull) break;                               // every stream of the wavefront is done
        const bool live0 = f0 < f_end, live1 = f1 < f_end;
        cf ga1[NBIN], ga2[NBIN];                                               // G1, G2 of frame f0 at the lane's bins
        float ny1a = 0.0f, ny2a = 0.0f, ny1b = 0.0f, ny2b = 0.0f;              // ... and of both frames at the Nyquist bin (real; lane 0)
        cf R[NB][4], Z[E];
        cf h2[NBIN], h2m[NBIN];                                                // second transform's input: lower half, mirrored upper half
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool live = u ? live1 : live0;
#pragma unroll
            for (int bq = 0; bq < NB; ++bq)
#pragma unroll
                for (int c = 0; c < 4; ++c) R[bq][c] = raw[bq][c] * wv[m_of_in<N>(bq, c)];
            prefetch_frame<N>(raw, xb, yb, u ? f0 + 2 : f1, f_end, n_frames, hop, T, a);     // in flight during this transform
            const cf e = frame_energy<N>(R);
            const bool same = frame_same<N>(R, g, e);
            const float sinv2 = pack_gain<N>(R, same, e);
            wave_fft<N, false>(R, Z, fl);
#pragma unroll
            for (int i = 0; i < E; ++i) buf[pos_final<N>(i, a)] = Z[i];
            __builtin_amdgcn_wave_barrier();
            float fd = 0.0f, fy = 0.0f, fl = 0.0f;
            const float lm = live ? 1.0f : 0.0f;
#pragma unroll
            for (int j = 0; j < NBIN; ++j) {
                const int k = a + L * j;
                const cf z = buf[k], zc = buf[(N - k) & (N - 1)];
                const cf X2 = add_conj(z, zc), D = sub_conj(z, zc);
                const BinOut t = bin_terms(X2, D, same, sinv2, 4.0f * eps, c_log, fd, fy, fl);
                const bool dc = (j == 0) && (a == 0);                          // DC: real, not halved
                const float s1 = (dc ? 2.0f * lm : lm) * t.s1, s2 = (dc ? 2.0f * lm : lm) * t.s2;
                const cf g1 = X2 * s1, g2 = X2 * s2;
                if (u == 0) {
                    ga1[j] = g1;
                    ga2[j] = g2;
                } else {
                    place_pair<N>(R, buf, j, a, pair_h(dc, ga1[j], g1), mirror_h(ga1[j], g1));
                    h2[j] = pair_h(dc, ga2[j], g2);
                    h2m[j] = mirror_h(ga2[j], g2);
                }
            }
            if (a == 0) {                                                       // Nyquist bin: real, not halved
                const cf z = buf[N / 2];
                const cf X2 = {2.0f * z.x, 0.0f}, D = {0.0f, 2.0f * z.y};
                const BinOut t = bin_terms(X2, D, same, sinv2, 4.0f * eps, c_log, fd, fy, fl);
                const float n1 = 2.0f * lm * t.s1 * X2.x, n2 = 2.0f * lm * t.s2 * X2.x;
                if (u == 0) { ny1a = n1; ny2a = n2; }
                else { ny1b = n1; ny2b = n2; }
            }
            if (live) {
                s[0] += (double)(0.25f * fd);
                s[1] += (double)(0.25f * fy);
                s[2] += (double)(0.5f * 0.69314718055994531f * fl);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- G1 of both frames: one inverse transform, overlap-add
        pair_finish<N>(R, buf, a, ny1a, ny1b);
        wave_fft<N, true>(R, Z, fl);
        asm volatile("" : "+v"(a));
        ring_add_and_flush<N>(op_smem, ring1_b, m1, Z, wv, f0, live0, live1, a, base, hop);
        // ---- G2
#pragma unroll
        for (int j = 0; j < NBIN; ++j) place_pair<N>(R, buf, j, a, h2[j], h2m[j]);
        pair_finish<N>(R, buf, a, ny2a, ny2b);
        wave_fft<N, true>(R, Z, fl);
        asm volatile("" : "+v"(a));
        ring_add_and_flush<N>(op_smem, ring2_b, m2, Z, wv, f0, live0, live1, a, base, hop);
        base = (base + 2 * hop) & (N - 1);
    }
    if (f_begin < f_end) ring_write_tail<N, 2>(ring1, tails, rg, b, run, f_end - f_begin, hop, a_);
    block_partials<3, MR_OPW>(s, red, b, part);
}

// ---- fold ---------------------------------------------------------------------------------------------------------
struct FoldRes { OlaGrad g; const float *alpha; };       // the two components of one resolution and its scalar
struct FoldArgs { FoldRes r[4]; int n_res; };

__global__ __launch_bounds__(256) void mr_fold_all_kernel(FoldArgs fa, int T, int accumulate, float *__restrict__ dx, long long ds)
{
    const int b = blockIdx.y, B = gridDim.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= T) return;
    float acc = 0.0f;
    for (int ri = 0; ri < fa.n_res; ++ri) {
        const FoldRes &r = fa.r[ri];
        float g[2] = {0.0f, 0.0f};
        for_padded_positions(n, r.g.N, T, [&](int p) { fold_pos<2>(r.g, B, b, p, g); });
        acc += r.alpha[0] * g[0] + g[1];
    }
    float *o = dx + (size_t)b * ds + n;
    *o = accumulate ? *o + acc : acc;
}

__global__ void mr_total_kernel(float *__restrict__ terms, int n_res, float w_sc, float w_log)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float tot = 0.0f;
    for (int r = 0; r < n_res; ++r) tot += w_sc * terms[2 * r] + w_log * terms[2 * r + 1];
    terms[2 * n_res] = tot / (float)n_res;
}

// value only
template <int N>
static int run_stats(const float *x, long long xs, const float *y, long long ys, const float *win, const float2 *tw, int B, int T,
                     int hop, float eps, float w_sc, float w_log, float res_scale, double *part, float *terms, float *coef,
                     hipStream_t st)
{
    const int n_frames = 1 + T / hop;
    const int groups = (n_frames + MR_FPG - 1) / MR_FPG;
    hipLaunchKernelGGL((mr_stats_kernel<N>), dim3(groups, B), dim3(WF<N>::WAVES * 64), 0, st, x, xs, y, ys, win, tw, T, hop,
                       n_frames, eps, part);
    const long long count = (long long)B * n_frames * (N / 2 + 1);
    hipLaunchKernelGGL(mr_finish_kernel, dim3(1), dim3(256), 0, st, part, groups * B, count, w_sc, w_log, res_scale, terms, coef);
    return mx_launch_status();
}

// value + the two time-domain gradient components of one resolution; fr describes what the fold pass needs
template <int N>
static int run_onepass(const float *x, long long xs, const float *y, long long ys, const float *win, const float2 *tw, int B, int T,
                       int hop, float eps, float w_sc, float w_log, float res_scale, double *part, float *terms, float *alpha,
                       float *ws, const OlaRuns &rg, FoldRes &fr, hipStream_t st)
{
    const int groups = (rg.n_runs + OP<N>::STREAMS - 1) / OP<N>::STREAMS;
    float *main1 = ws, *main2 = main1 + ola_main_floats(B, rg, hop), *tails = main2 + ola_main_floats(B, rg, hop);
    const long long count = (long long)B * rg.n_frames * (N / 2 + 1);
    const float c_log = (float)((double)res_scale * w_log / (double)count);
    static MxLdsLatch latch = {};                              // one per N, as the kernel is
    if (mx_set_dyn_lds(latch, reinterpret_cast<const void *>(&mr_onepass_kernel<N>), OP<N>::lds_bytes()) != MX_OK)
        return MX_ERR_LAUNCH;
    hipLaunchKernelGGL((mr_onepass_kernel<N>), dim3(groups, B), dim3(MR_OPW * 64), OP<N>::lds_bytes(), st, x, xs, y, ys, win, tw, T,
                       hop, rg, eps, c_log, part, main1, main2, tails);
    hipLaunchKernelGGL(mr_finish_kernel, dim3(1), dim3(256), 0, st, part, groups * B, count, w_sc, w_log, res_scale, terms, alpha);
    fr = FoldRes{OlaGrad{main1, tails, N, hop, rg}, alpha};
    return mx_launch_status();
}

// y_hat, y: B rows of T samples (row strides); n_res resolutions with fft_sizes in {512,1024,2048} and hops
// given as HOST arrays (the only host pointers of this ABI: they select kernel instantiations and grids);
// windows (n_res, 2048): row r holds the n_fft-long window of resolution r (win_length hann, centred);
// twiddle (2048,2) = exp(-2 pi i m / 2048).  terms (2*n_res + 1): [sc_0, logmag_0, ..., total].
// dx (B rows, stride dx_stride) = d total / d y_hat, or NULL.  Workspaces: part (doubles) >= 3 * B *
// max_r ceil(frames_r / 8); coef (n_res,) floats (alpha_r); scratch (floats, only when dx != NULL) >= sum_r 2 * B *
// (frames_r * hop_r + runs_r * max(n_fft_r - hop_r, 0)) with runs_r = ceil(frames_r / F_r), F_r = max(32, ceil(n_fft_r / hop_r))
// rounded up to even: the two time-domain gradient components of every resolution (run sums + run tails; ola_ring.h: ola_ws_floats).
MX_EXPORT int mx_mrstft_loss(const float *y_hat, int64_t y_hat_stride, const float *y, int64_t y_stride, int64_t B,
                             int64_t T, int32_t n_res, const int32_t *fft_sizes, const int32_t *hops,
                             const float *windows, const float *twiddle, float w_sc, float w_log, float eps,
                             double *part, float *coef, float *scratch, float *terms, float *dx,
                             int64_t dx_stride, void *stream)
{
    if (!y_hat || !y || !fft_sizes || !hops || !windows || !twiddle || !part || !coef || !terms || B <= 0 || T <= 0 ||
        n_res <= 0 || (dx && !scratch))
        return MX_ERR_ARG;
    if (B > 65535 || T >= (1ll << 30)) return MX_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const float res_scale = 1.0f / (float)n_res;
    FoldArgs fa;
    fa.n_res = 0;
    int folded = 0;
    float *ws = scratch;
    for (int r = 0; r < n_res; ++r) {
        const int N = fft_sizes[r], hop = hops[r];
        if (T <= N / 2 || hop <= 0) return MX_ERR_UNSUPPORTED;
        const float *win = windows + (size_t)r * MR_MAXN;
        const OlaRuns rg = ola_runs(N, hop, (int)T);
        int rc;
#define MR_RUN(NN)                                                                                                              \
    rc = dx ? run_onepass<NN>(y_hat, (long long)y_hat_stride, y, (long long)y_stride, win, (const float2 *)twiddle, (int)B,     \
                              (int)T, hop, eps, w_sc, w_log, res_scale, part, terms + 2 * r, coef + r, ws, rg, fa.r[fa.n_res], st) \
            : run_stats<NN>(y_hat, (long long)y_hat_stride, y, (long long)y_stride, win, (const float2 *)twiddle, (int)B,      \
                            (int)T, hop, eps, w_sc, w_log, res_scale, part, terms + 2 * r, coef + r, st)
        if (N == 512) MR_RUN(512);
        else if (N == 1024) MR_RUN(1024);
        else if (N == 2048) MR_RUN(2048);
        else return MX_ERR_UNSUPPORTED;
#undef MR_RUN
        if (rc != MX_OK) return rc;
        if (dx) {
            ws += ola_ws_floats(2, (int)B, rg, hop);
            if (++fa.n_res == 4 || r == n_res - 1) {
                hipLaunchKernelGGL(mr_fold_all_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, st, fa, (int)T,
                                   folded, dx, (long long)dx_stride);
                folded = 1;
                fa.n_res = 0;
            }
        }
    }
    hipLaunchKernelGGL(mr_total_kernel, dim3(1), dim3(64), 0, st, terms, (int)n_res, w_sc, w_log);
    return mx_launch_status();
}
