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
//   onepass : a STREAM (64 lanes; 32 for N = 512, two streams per wavefront) walks a RUN of F consecutive frames of one
//             clip, two frames at a time: forward FFT of x + i*s*y per frame (register-staged radix-4 Stockham, see below)
//             -> both spectra by Hermitian separation -> loss sums and the frame's G1, G2; the pair's G1 spectra are
//             completed to Hermitian ones and go through ONE inverse FFT as G1~_a + i G1~_b (real / imaginary part = the
//             two frames' time-domain gradients), likewise G2: two transforms per frame (it was 1.5, plus 24 B per bin
//             of traffic).  The windowed frames are overlap-added in two stream-private LDS rings of N floats; after a
//             frame is added its first `hop` positions are final (within the run) and leave for memory; at the end of the
//             run the ring's remaining N - hop positions leave as the run's TAIL.
//   finish  : loss terms and alpha_r from the per-workgroup partial sums
//   fold    : dx[n] = sum_r sum_{padded positions p of n} ( alpha_r g1_r[p] + g2_r[p] ),  g[p] = run sums + the tails of the
//             (<= 2) earlier runs that reach p -- a gather: deterministic, no atomics
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
#include "wave_fft.h"
#include "spectral_pair.h"

#define MR_FPG 16        // frames per workgroup (value-only pass); the partial-sum workspace is sized for >= 8
#ifndef MR_RUN_MIN
#define MR_RUN_MIN 32    // frames per run of the one-pass kernel (at least ceil(N / hop): a position then lies in at most two earlier runs' tails)
#endif
#define MR_OPW 4         // wavefronts per workgroup of the one-pass kernel
#ifndef MR_OP_EU
#define MR_OP_EU 2       // waves per SIMD the 512 / 1024 one-pass kernels are compiled for (2048: 1, its LDS leaves one workgroup per CU)
#endif

// tw_s[m] = exp(-2 pi i m / N) from the 2048-point table in global memory, once per workgroup
template <int N>
__device__ __forceinline__ void stage_twiddles(cf *tw_s, const float2 *__restrict__ tw)
{
    for (int m = threadIdx.x; m < N; m += WF<N>::WAVES * 64) {
        const float2 w = tw[m * (MR_MAXN / N)];
        tw_s[m] = {w.x, w.y};
    }
    __syncthreads();
}

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

// the same with the lane's window values in registers (wv[m] = win[a + L m]; stage-A register (b, c) sits at m = b + (N/4/L) c)
template <int N, bool INTERIOR>
__device__ __forceinline__ void load_frame_w(cf (&R)[WF<N>::NB][4], const float *xb, const float *yb, const float (&wv)[WF<N>::E],
                                             int f, int hop, int T, int a)
{
    const float *xf = xb + (f * hop - N / 2 + a), *yf = yb + (f * hop - N / 2 + a);     // dereferenced only when INTERIOR
#pragma unroll
    for (int b = 0; b < WF<N>::NB; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float w = wv[b + (N / 4 / WF<N>::L) * c];
            if (INTERIOR) {
                R[b][c] = {xf[WF<N>::L * b + (N / 4) * c] * w, yf[WF<N>::L * b + (N / 4) * c] * w};
            } else {
                const int s = reflect_index(f * hop + a + WF<N>::L * b + (N / 4) * c - N / 2, T);
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
    __shared__ double red[WAVES][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / L, a_ = lane % L;
    const int b = blockIdx.y;
    const float *xb = x + (size_t)b * xs, *yb = y + (size_t)b * ys;
    cf *buf = xbuf[wave * FW + g];
    stage_twiddles<N>(tw_s, tw);
    FftLane<N> fl;
    fft_lane_setup<N>(fl, buf, tw_s, tw, a_);
    double s_d = 0.0, s_y = 0.0, s_l = 0.0;
    for (int it = 0; it < MR_FPG / (WAVES * FW); ++it) {
        int a = a_;                                                      // opaque per iteration: see mr_grad_kernel
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
            s_d += (double)fd;
            s_y += (double)fy;
            s_l += (double)(0.5f * 0.69314718055994531f * fl);
        }
        __builtin_amdgcn_wave_barrier();
    }
    s_d = wave_sum_f64(s_d); s_y = wave_sum_f64(s_y); s_l = wave_sum_f64(s_l);
    if (lane == 0) { red[wave][0] = s_d; red[wave][1] = s_y; red[wave][2] = s_l; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double acc = 0.0;
        for (int w = 0; w < WAVES; ++w) acc += red[w][threadIdx.x];
        part[((size_t)b * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = acc;
    }
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
// window position index m of a lane: position a + L m.  Stage-A register (b, c) and final result i sit at these m:
template <int N> __device__ __forceinline__ constexpr int m_of_in(int b, int c) { return b + (N / 4 / WF<N>::L) * c; }
template <int N> __device__ __forceinline__ constexpr int m_of_out(int i) { return (pos_final<N>(i, 0)) / WF<N>::L; }

template <int N>
__global__ __launch_bounds__(MR_OPW * 64) __attribute__((amdgpu_waves_per_eu(N == 2048 ? 1 : MR_OP_EU))) void mr_onepass_kernel(
    const float *__restrict__ x, long long xs, const float *__restrict__ y, long long ys, const float *__restrict__ win,
    const float2 *__restrict__ tw, int T, int hop, int n_frames, int F, int n_runs, float eps, float c_log,
    double *__restrict__ part, float *__restrict__ main1, float *__restrict__ main2, float *__restrict__ tails)
{
    constexpr int L = OP<N>::L, E = OP<N>::E, NB = OP<N>::NB, FW = OP<N>::FW, STREAMS = OP<N>::STREAMS, NBIN = OP<N>::NBIN;
    extern __shared__ __attribute__((aligned(16))) unsigned char op_smem[];
    // rings first: ring c of stream s starts at byte (2 s + c) 4 N, so that a slot's address is (position bytes & (4 N - 1)) | base
    float *rings = reinterpret_cast<float *>(op_smem);
    cf *tw_s = reinterpret_cast<cf *>(op_smem + (size_t)STREAMS * 2 * N * 4);
    cf *xbuf = reinterpret_cast<cf *>(op_smem + (size_t)STREAMS * 2 * N * 4 + (size_t)N * 8);
    double *red = reinterpret_cast<double *>(op_smem + (size_t)N * 8 + (size_t)STREAMS * WF<N>::LEN * 8 + (size_t)STREAMS * 2 * N * 4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane / L, a_ = lane % L;
    const int b = blockIdx.y, sidx = wave * FW + g;
    const float *xb = x + (size_t)b * xs, *yb = y + (size_t)b * ys;
    cf *buf = xbuf + (size_t)sidx * WF<N>::LEN;
    float *ring1 = rings + (size_t)sidx * 2 * N, *ring2 = ring1 + N;
    for (int m = threadIdx.x; m < N; m += MR_OPW * 64) {
        const float2 w = tw[m * (MR_MAXN / N)];
        tw_s[m] = {w.x, w.y};
    }
    for (int j = a_; j < 2 * N; j += L) ring1[j] = 0.0f;
    __syncthreads();
    FftLane<N> fl;
    fft_lane_setup<N>(fl, buf, tw_s, tw, a_);

    const int run = blockIdx.x * STREAMS + sidx;
    const int f_begin = run * F, f_end = min(f_begin + F, n_frames);          // (an idle stream: f_begin >= f_end)
    const int tail_len = N > hop ? N - hop : 0;
    float wv[E];                                                              // the lane's window values: positions a + L m
#pragma unroll
    for (int m = 0; m < E; ++m) wv[m] = win[a_ + L * m];
    double s_d = 0.0, s_y = 0.0, s_l = 0.0;
    int base = 0;                                                             // ring slot of the current frame's position 0

    // The pair's windowed gradient frames (real part: frame f0 at ring position bs, imaginary part: frame f1 at bs + hop) ->
    // ring: read - add - write, 16 / 32 values a lane (LDS operations of a wave execute in order); after each frame its first
    // `hop` positions are final within the run and leave the ring for memory.  A slot's byte address is
    // ((position bytes) & (4 N - 1)) | ring base: two vector instructions per value.
    auto add_and_flush = [&](unsigned ring_b, float *mainp, const cf (&Z)[E], int f0, bool live0, bool live1, int a, int bs) {
        unsigned char *const lds = op_smem;
        cf Zw[E];
#pragma unroll
        for (int i = 0; i < E; ++i) Zw[i] = Z[i] * wv[m_of_out<N>(i)];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = f0 + u;
            const bool live = u ? live1 : live0;
            const unsigned tb = (unsigned)(((u ? bs + hop : bs) + a) * 4);
            if (live) {
                float old[E];
#pragma unroll
                for (int i = 0; i < E; ++i)
                    old[i] = *reinterpret_cast<const float *>(lds + (((tb + 4u * (unsigned)pos_final<N>(i, 0)) & (4u * N - 1u)) | ring_b));
#pragma unroll
                for (int i = 0; i < E; ++i)
                    *reinterpret_cast<float *>(lds + (((tb + 4u * (unsigned)pos_final<N>(i, 0)) & (4u * N - 1u)) | ring_b)) =
                        old[i] + (u ? Zw[i].y : Zw[i].x);
            }
            __builtin_amdgcn_wave_barrier();
            if (live) {
                float *o = mainp + (size_t)f * hop;
                for (int j = a; j < hop; j += L) {
                    float v = 0.0f;
                    if (j < N) {
                        float *slot = reinterpret_cast<float *>(lds + (((tb + 4u * (unsigned)(j - a)) & (4u * N - 1u)) | ring_b));
                        v = *slot;
                        *slot = 0.0f;
                    }
                    o[j] = v;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    };
    const unsigned ring1_b = (unsigned)(sidx * 2) * 4u * N, ring2_b = ring1_b + 4u * N;

    float *m1 = main1 + (size_t)b * n_frames * hop, *m2 = main2 + (size_t)b * n_frames * hop;
#ifndef MR_PREFETCH
#define MR_PREFETCH 1     // the samples of a frame are requested while the frame before it is transformed (0: loaded where they are used)
#endif
    // Round 6: a wave spent 31 % of its cycles in s_waitcnt (profiles/r06): every frame began with 2 E global loads whose L2 round trip
    // nothing covered.  `raw` holds the next frame's unwindowed samples; the window multiplication is the same one, a frame later.
    cf raw[NB][4];
    auto fetch = [&](int f, int a) {
        const int fl_ = f < f_end ? f : (n_frames - 1);                        // dead slots transform a valid frame and contribute nothing
        // interior (decided for the whole wavefront: a per-position test would put every load in a basic block of its own):
        // no position of the frame needs the reflection arithmetic, the loads are one base pointer + constant offsets
        const bool inter_lane = fl_ * hop - N / 2 >= 0 && fl_ * hop + N / 2 <= T;
        if (__ballot(!inter_lane) == 0ull) fetch_frame<N, true>(raw, xb, yb, fl_, hop, T, a);
        else fetch_frame<N, false>(raw, xb, yb, fl_, hop, T, a);
    };
    if (MR_PREFETCH) fetch(f_begin, a_);
    for (int fp = 0; fp < F; fp += 2) {
        // the lane's position is made opaque to the optimiser again before every transform: the ~100 twiddle / exchange /
        // window addresses built from it would otherwise be shared by the iteration's four transforms (and hoisted out of the
        // frame loop) and live in scratch memory (21 / 30 spilled registers for N = 1024 / 2048)
#ifndef MR_NO_OPAQUE
#define MR_OPAQUE(v) asm volatile("" : "+v"(v))
#else
#define MR_OPAQUE(v)
#endif
        int a = a_;
        asm volatile("" : "+v"(a));
        const int f0 = f_begin + fp, f1 = f0 + 1;
        if (__ballot(f0 < f_end) == 0ull) break;                               // every stream of the wavefront is done
        const bool live0 = f0 < f_end, live1 = f1 < f_end;
        cf ga1[NBIN], ga2[NBIN];                                               // G1, G2 of frame f0 at the lane's bins
        float ny1a = 0.0f, ny2a = 0.0f;                                        // ... and at the Nyquist bin (real; lane 0)
        cf R[NB][4], Z[E];
        cf h2[NBIN], h2m[NBIN];                                                // second transform's input: lower half, mirrored upper half
        float h2ny_re = 0.0f, h2ny_im = 0.0f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = u ? f1 : f0;
            const bool live = u ? live1 : live0;
            const int fl_ = live ? f : (n_frames - 1);                         // dead slots transform a valid frame and contribute nothing
            if (MR_PREFETCH) {
#pragma unroll
                for (int bq = 0; bq < NB; ++bq)
#pragma unroll
                    for (int c = 0; c < 4; ++c) R[bq][c] = raw[bq][c] * wv[bq + (N / 4 / L) * c];
                fetch(u ? f0 + 2 : f1, a);                                     // the frame after this one, in flight during this transform
            } else {
                // interior (decided for the whole wavefront: a per-position test would put every load in a basic block of its own):
                // no position of the frame needs the reflection arithmetic, the loads are one base pointer + constant offsets
                const bool inter_lane = fl_ * hop - N / 2 >= 0 && fl_ * hop + N / 2 <= T;
                if (__ballot(!inter_lane) == 0ull) load_frame_w<N, true>(R, xb, yb, wv, fl_, hop, T, a);
                else load_frame_w<N, false>(R, xb, yb, wv, fl_, hop, T, a);
            }
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
                    // H = G~_a + i G~_b of the pair at position k (lower half) and its mirror image conj G~_a + i conj G~_b at N - k
                    const cf p1 = ga1[j], p2 = ga2[j];
                    R[j % NB][j / NB] = dc ? cf{p1.x, g1.x} : add_pi(p1, g1);
                    buf[N - k] = mirror_h(p1, g1);                              // (k = 0 lands in the pad: never read)
                    h2[j] = dc ? cf{p2.x, g2.x} : add_pi(p2, g2);
                    h2m[j] = mirror_h(p2, g2);
                }
            }
            if (a == 0) {                                                       // Nyquist bin: real, not halved
                const cf z = buf[N / 2];
                const cf X2 = {2.0f * z.x, 0.0f}, D = {0.0f, 2.0f * z.y};
                const BinOut t = bin_terms(X2, D, same, sinv2, 4.0f * eps, c_log, fd, fy, fl);
                const float n1 = 2.0f * lm * t.s1 * X2.x, n2 = 2.0f * lm * t.s2 * X2.x;
                if (u == 0) { ny1a = n1; ny2a = n2; }
                else { buf[N / 2] = {ny1a, n1}; h2ny_re = ny2a; h2ny_im = n2; }
            }
            if (live) {
                s_d += (double)(0.25f * fd);
                s_y += (double)(0.25f * fy);
                s_l += (double)(0.5f * 0.69314718055994531f * fl);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- G1 of both frames: one inverse transform, overlap-add
#pragma unroll
        for (int bq = 0; bq < NB; ++bq)
#pragma unroll
            for (int c = 2; c < 4; ++c) R[bq][c] = buf[a + L * bq + (N / 4) * c];
        __builtin_amdgcn_wave_barrier();
        wave_fft<N, true>(R, Z, fl);
        MR_OPAQUE(a);
        add_and_flush(ring1_b, m1, Z, f0, live0, live1, a, base);
        // ---- G2
#pragma unroll
        for (int j = 0; j < NBIN; ++j) {
            R[j % NB][j / NB] = h2[j];
            buf[N - (a + L * j)] = h2m[j];
        }
        if (a == 0) buf[N / 2] = {h2ny_re, h2ny_im};
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int bq = 0; bq < NB; ++bq)
#pragma unroll
            for (int c = 2; c < 4; ++c) R[bq][c] = buf[a + L * bq + (N / 4) * c];
        __builtin_amdgcn_wave_barrier();
        wave_fft<N, true>(R, Z, fl);
        MR_OPAQUE(a);
        add_and_flush(ring2_b, m2, Z, f0, live0, live1, a, base);
        base = (base + 2 * hop) & (N - 1);
    }
    // the run's tail: positions [f_end * hop, f_end * hop + N - hop) as far as this run's frames reach them
    if (f_begin < f_end) {
        const int bs = ((f_end - f_begin) * hop) & (N - 1);
        float *t1 = tails + ((size_t)b * n_runs + run) * 2 * tail_len, *t2 = t1 + tail_len;
        for (int j = a_; j < tail_len; j += L) {
            t1[j] = ring1[(bs + j) & (N - 1)];
            t2[j] = ring2[(bs + j) & (N - 1)];
        }
    }
    s_d = wave_sum_f64(s_d); s_y = wave_sum_f64(s_y); s_l = wave_sum_f64(s_l);
    if (lane == 0) { red[wave * 3] = s_d; red[wave * 3 + 1] = s_y; red[wave * 3 + 2] = s_l; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double acc = 0.0;
        for (int w = 0; w < MR_OPW; ++w) acc += red[w * 3 + threadIdx.x];
        part[((size_t)b * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = acc;
    }
}

// ---- fold ---------------------------------------------------------------------------------------------------------
struct FoldRes {
    const float *main1, *main2, *tails, *alpha;       // (B, n_frames * hop) x 2, (B, n_runs, 2, tail_len), scalar
    int N, hop, n_frames, F, n_runs, tail_len;
};
struct FoldArgs { FoldRes r[4]; int n_res; };

// g1, g2 of resolution r at padded position p of clip b: the run sums plus the tails of the runs that end before p and reach it
__device__ __forceinline__ void fold_pos(const FoldRes &r, int b, int p, float &g1, float &g2)
{
    const int flushed = r.n_frames * r.hop;
    if (p < flushed) {
        g1 += r.main1[(size_t)b * flushed + p];
        g2 += r.main2[(size_t)b * flushed + p];
    }
    if (r.tail_len == 0) return;
    int rho = p / (r.F * r.hop);
    if (rho > r.n_runs - 1) rho = r.n_runs - 1;
    for (int q = rho; q >= 0 && q >= rho - 2; --q) {
        int fe = (q + 1) * r.F;
        if (fe > r.n_frames) fe = r.n_frames;
        const int j = p - fe * r.hop;
        if (j >= 0 && j < r.tail_len) {
            const float *t = r.tails + ((size_t)b * r.n_runs + q) * 2 * r.tail_len;
            g1 += t[j];
            g2 += t[r.tail_len + j];
        }
    }
}

__global__ __launch_bounds__(256) void mr_fold_all_kernel(FoldArgs fa, int T, int accumulate, float *__restrict__ dx, long long ds)
{
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= T) return;
    float acc = 0.0f;
    for (int ri = 0; ri < fa.n_res; ++ri) {
        const FoldRes &r = fa.r[ri];
        const int N = r.N;
        float g1 = 0.0f, g2 = 0.0f;
        // padded positions that map to sample n: the direct one and up to two reflected ones
        fold_pos(r, b, n + N / 2, g1, g2);
        if (n >= 1 && n <= N / 2) fold_pos(r, b, N / 2 - n, g1, g2);
        if (n <= T - 2 && n >= T - 1 - N / 2) fold_pos(r, b, N / 2 + 2 * (T - 1) - n, g1, g2);
        acc += r.alpha[0] * g1 + g2;
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

static int mr_run_frames(int N, int hop)
{
    int F = (N + hop - 1) / hop;
    if (F < MR_RUN_MIN) F = MR_RUN_MIN;
    return (F + 1) & ~1;
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
                       float *ws, FoldRes &fr, hipStream_t st)
{
    const int n_frames = 1 + T / hop;
    const int F = mr_run_frames(N, hop), n_runs = (n_frames + F - 1) / F, tail_len = N > hop ? N - hop : 0;
    const int groups = (n_runs + OP<N>::STREAMS - 1) / OP<N>::STREAMS;
    float *main1 = ws, *main2 = main1 + (size_t)B * n_frames * hop, *tails = main2 + (size_t)B * n_frames * hop;
    const long long count = (long long)B * n_frames * (N / 2 + 1);
    const float c_log = (float)((double)res_scale * w_log / (double)count);
    static MxLdsLatch latch = {};                              // one per N, as the kernel is
    if (mx_set_dyn_lds(latch, reinterpret_cast<const void *>(&mr_onepass_kernel<N>), OP<N>::lds_bytes()) != MX_OK)
        return MX_ERR_LAUNCH;
    hipLaunchKernelGGL((mr_onepass_kernel<N>), dim3(groups, B), dim3(MR_OPW * 64), OP<N>::lds_bytes(), st, x, xs, y, ys, win, tw, T,
                       hop, n_frames, F, n_runs, eps, c_log, part, main1, main2, tails);
    hipLaunchKernelGGL(mr_finish_kernel, dim3(1), dim3(256), 0, st, part, groups * B, count, w_sc, w_log, res_scale, terms, alpha);
    fr = FoldRes{main1, main2, tails, alpha, N, hop, n_frames, F, n_runs, tail_len};
    return mx_launch_status();
}

// floats of workspace one resolution needs for the gradient (mirrored by mod_extraction_amd/mrstft.py)
static size_t mr_ws_floats(int B, int T, int N, int hop)
{
    const int n_frames = 1 + T / hop, F = mr_run_frames(N, hop), n_runs = (n_frames + F - 1) / F, tail_len = N > hop ? N - hop : 0;
    return 2 * (size_t)B * ((size_t)n_frames * hop + (size_t)n_runs * tail_len);
}

// y_hat, y: B rows of T samples (row strides); n_res resolutions with fft_sizes in {512,1024,2048} and hops
// given as HOST arrays (the only host pointers of this ABI: they select kernel instantiations and grids);
// windows (n_res, 2048): row r holds the n_fft-long window of resolution r (win_length hann, centred);
// twiddle (2048,2) = exp(-2 pi i m / 2048).  terms (2*n_res + 1): [sc_0, logmag_0, ..., total].
// dx (B rows, stride dx_stride) = d total / d y_hat, or NULL.  Workspaces: part (doubles) >= 3 * B *
// max_r ceil(frames_r / 8); coef (n_res,) floats (alpha_r); scratch (floats, only when dx != NULL) >= sum_r 2 * B *
// (frames_r * hop_r + runs_r * max(n_fft_r - hop_r, 0)) with runs_r = ceil(frames_r / F_r), F_r = max(32, ceil(n_fft_r / hop_r))
// rounded up to even: the two time-domain gradient components of every resolution (run sums + run tails).
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
        int rc;
#define MR_RUN(NN)                                                                                                              \
    rc = dx ? run_onepass<NN>(y_hat, (long long)y_hat_stride, y, (long long)y_stride, win, (const float2 *)twiddle, (int)B,     \
                              (int)T, hop, eps, w_sc, w_log, res_scale, part, terms + 2 * r, coef + r, ws, fa.r[fa.n_res], st) \
            : run_stats<NN>(y_hat, (long long)y_hat_stride, y, (long long)y_stride, win, (const float2 *)twiddle, (int)B,      \
                            (int)T, hop, eps, w_sc, w_log, res_scale, part, terms + 2 * r, coef + r, st)
        if (N == 512) MR_RUN(512);
        else if (N == 1024) MR_RUN(1024);
        else if (N == 2048) MR_RUN(2048);
        else return MX_ERR_UNSUPPORTED;
#undef MR_RUN
        if (rc != MX_OK) return rc;
        if (dx) {
            ws += mr_ws_floats((int)B, (int)T, N, hop);
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
