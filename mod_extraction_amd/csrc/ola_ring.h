// ola_ring.h -- the one-pass gradient pipeline of the spectral losses: frames in, time-domain gradient out, nothing per bin in
// memory.  Users: the MR-STFT loss (mrstft.hip, C = 2 gradient components) and the log-mel L1 loss (logmel_loss.hip, C = 1); they
// supply the per-bin mathematics, everything between the bins and dx is here.
//   runs   : a clip's n_frames = 1 + T / hop frames are cut into n_runs RUNS of F consecutive frames.  A STREAM (the L lanes that
//            hold one frame: 64; 32 for N = 512, two streams per wavefront) walks one run, two frames at a time, and prefetches a
//            frame while the frame before it is transformed (prefetch_frame).
//   pair   : the two frames' gradient spectra are completed to Hermitian ones and go through ONE inverse transform as
//            G~_a + i G~_b: real / imaginary part = the two frames' time-domain gradients (pair_h, place_pair, pair_finish).
//   ring   : the windowed frames are overlap-added in a stream-private LDS ring of N floats per component.  After a frame is added
//            its first `hop` positions are final WITHIN THE RUN and leave for memory (the run sums, `main`: (C, B, n_frames * hop),
//            frame f at f * hop); at the end of the run the ring's remaining tail_len = N - hop positions leave as the run's TAIL
//            ((B, n_runs, C, tail_len)): what this run adds to positions that later runs flush (ring_add_and_flush, ring_write_tail).
//   fold   : dx[n] = sum over the padded positions p of n (for_padded_positions) of g[p],  g[p] = run sums + the tails of the
//            earlier runs that reach p (fold_pos) -- a gather: deterministic, no atomics.
// Invariants:
//   * F >= ceil(N / hop): a tail (tail_len < N <= F hop positions) ends within the run after its own.  Position p, in run
//     rho = min(p / (F hop), n_runs - 1), is then reached by the tail of run rho - 1 and, past the clip's last flushed position,
//     by the (short) last run's own: a position lies in at most two tails, and fold_pos looks at rho, rho - 1 and rho - 2.
//     F is even: frames go through the inverse transform in pairs.
//   * the rings lie first in the dynamic LDS, ring r at byte r * 4 N, so that a slot's byte address is
//     (position bytes & (4 N - 1)) | ring base: two vector instructions per value.
//   * LDS operations of a wavefront execute in order and a ring belongs to one stream: no barrier beyond the compiler's
//     (wave_barrier) between a frame's add and its flush.
// Everything here is forced inline and takes the lane's register arrays by reference: as a call, or not fully unrolled, they
// would live in scratch memory.  No floating-point expression may be reordered (the users are built with -ffp-contract=off).
#pragma once
#include "wave_fft.h"
#include "spectral_pair.h"

#ifndef OLA_RUN_MIN
#define OLA_RUN_MIN 32   // frames per run at least (tools/exp_mrstft.py builds variants); mod_extraction_amd/mrstft.py: RUN_MIN
#endif

// ---- run geometry (the only definition: mod_extraction_amd/mrstft.py run_geometry restates it for the workspace sizes) ----------
struct OlaRuns { int n_frames, F, n_runs, tail_len; };
__host__ __device__ __forceinline__ OlaRuns ola_runs(int N, int hop, int T)
{
    OlaRuns g;
    g.n_frames = 1 + T / hop;
    int F = (N + hop - 1) / hop;
    if (F < OLA_RUN_MIN) F = OLA_RUN_MIN;
    g.F = (F + 1) & ~1;
    g.n_runs = (g.n_frames + g.F - 1) / g.F;
    g.tail_len = N > hop ? N - hop : 0;
    return g;
}
// floats of workspace for C components of B clips: the run sums, then the tails
__host__ __device__ __forceinline__ size_t ola_main_floats(int B, const OlaRuns &g, int hop) { return (size_t)B * g.n_frames * hop; }
__host__ __device__ __forceinline__ size_t ola_ws_floats(int C, int B, const OlaRuns &g, int hop)
{
    return (size_t)C * (ola_main_floats(B, g, hop) + (size_t)B * g.n_runs * g.tail_len);
}

// window position index m of a lane: position a + L m.  Stage-A register (b, c) and final result i sit at these m:
template <int N> __device__ __forceinline__ constexpr int m_of_in(int b, int c) { return b + (N / 4 / WF<N>::L) * c; }
template <int N> __device__ __forceinline__ int m_of_out(int i) { return pos_final<N>(i, 0) / WF<N>::L; }

// tw_s[m] = exp(-2 pi i m / N) from a table of N * TWS points in global memory (TWS as for fft_lane_setup), by the NT threads of
// the workgroup; the caller's next __syncthreads publishes it
template <int N, int TWS, int NT>
__device__ __forceinline__ void stage_twiddles(cf *tw_s, const float2 *__restrict__ tw)
{
    for (int m = threadIdx.x; m < N; m += NT) {
        const float2 w = tw[m * TWS];
        tw_s[m] = {w.x, w.y};
    }
}

// ---- frame prefetch -------------------------------------------------------------------------------------------------------------
// raw = the unwindowed samples of frame f of the run that ends at f_end (a dead slot, f >= f_end, transforms a valid frame and
// contributes nothing).  Interior is decided for the whole wavefront (a per-position test would put every load in a basic block
// of its own): no position of the frame needs the reflection arithmetic, the loads are one base pointer + constant offsets.
// Round 6: a wave spent 31 % of its cycles in s_waitcnt (profiles/r06) while every frame began with 2 E global loads whose L2
// round trip nothing covered; requested a frame ahead, the window multiplication is the same one, a frame later.
template <int N>
__device__ __forceinline__ void prefetch_frame(cf (&raw)[WF<N>::NB][4], const float *xb, const float *yb, int f, int f_end,
                                               int n_frames, int hop, int T, int a)
{
    const int fl_ = f < f_end ? f : (n_frames - 1);
    const bool inter_lane = fl_ * hop - N / 2 >= 0 && fl_ * hop + N / 2 <= T;
    if (__ballot(!inter_lane) == 0ull) fetch_frame<N, true>(raw, xb, yb, fl_, hop, T, a);
    else fetch_frame<N, false>(raw, xb, yb, fl_, hop, T, a);
}

// ---- Hermitian pair packing -----------------------------------------------------------------------------------------------------
// G~_a, G~_b: the halved gradient spectra of the pair's frames at the lane's bins k = a + L j, j < N / 2 / L (DC: not halved,
// real), and at the Nyquist bin on lane 0 (not halved, real).
// H = G~_a + i G~_b at bin k of the lower half; its mirror image at N - k is mirror_h(G~_a, G~_b) = conj G~_a + i conj G~_b
__device__ __forceinline__ cf pair_h(bool dc, cf ga, cf gb) { return dc ? cf{ga.x, gb.x} : add_pi(ga, gb); }
// bin j of the lane: H into the stage-A register that holds position k, the mirror image into the exchange buffer
// (k = 0 lands in the pad: never read)
template <int N>
__device__ __forceinline__ void place_pair(cf (&R)[WF<N>::NB][4], cf *buf, int j, int a, cf h, cf hm)
{
    R[j % WF<N>::NB][j / WF<N>::NB] = h;
    buf[N - (a + WF<N>::L * j)] = hm;
}
// the Nyquist bin, then columns 2..3 of the stage-A registers (positions N / 2 .. N - 1) from the exchange buffer
template <int N>
__device__ __forceinline__ void pair_finish(cf (&R)[WF<N>::NB][4], cf *buf, int a, float ny_a, float ny_b)
{
    if (a == 0) buf[N / 2] = {ny_a, ny_b};
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int bq = 0; bq < WF<N>::NB; ++bq)
#pragma unroll
        for (int c = 2; c < 4; ++c) R[bq][c] = buf[a + WF<N>::L * bq + (N / 4) * c];
    __builtin_amdgcn_wave_barrier();
}

// ---- ring -----------------------------------------------------------------------------------------------------------------------
// Z: the inverse transform of a pair (real part: frame f0 at ring position bs, imaginary part: frame f0 + 1 at bs + hop); wv: the
// lane's window values (positions a + L m).  Window, then per frame: read ALL - add - write ALL, 16 / 32 values a lane; the
// frame's first `hop` positions leave for mainp (this clip's run sums of the component) and are zeroed.  lds: the start of the
// dynamic LDS; ring_b: the ring's byte offset in it.
template <int N>
__device__ __forceinline__ void ring_add_and_flush(unsigned char *lds, unsigned ring_b, float *mainp, const cf (&Z)[WF<N>::E],
                                                   const float (&wv)[WF<N>::E], int f0, bool live0, bool live1, int a, int bs, int hop)
{
    constexpr int L = WF<N>::L, E = WF<N>::E;
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
}

// the tail of run `run` of clip b after `done` frames: positions [done * hop, done * hop + tail_len) of the run, as far as its
// frames reach them, from the stream's C consecutive rings
template <int N, int C>
__device__ __forceinline__ void ring_write_tail(const float *ring, float *__restrict__ tails, const OlaRuns &g, int b, int run,
                                                int done, int hop, int a)
{
    const int bs = (done * hop) & (N - 1);
    float *t = tails + ((size_t)b * g.n_runs + run) * C * g.tail_len;
    for (int j = a; j < g.tail_len; j += WF<N>::L)
#pragma unroll
        for (int c = 0; c < C; ++c) t[c * g.tail_len + j] = ring[c * N + ((bs + j) & (N - 1))];
}

// ---- fold -----------------------------------------------------------------------------------------------------------------------
// one resolution's time-domain gradient components: run sums (C, B, n_frames * hop), tails (B, n_runs, C, tail_len)
struct OlaGrad {
    const float *main, *tails;
    int N, hop;
    OlaRuns g;
};
// acc[c] += component c at padded position p of clip b: the run sum plus the tails of the runs that end before p and reach it
template <int C>
__device__ __forceinline__ void fold_pos(const OlaGrad &r, int B, int b, int p, float (&acc)[C])
{
    const OlaRuns &g = r.g;
    const int flushed = g.n_frames * r.hop;
    if (p < flushed) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += r.main[((size_t)c * B + b) * flushed + p];
    }
    if (g.tail_len == 0) return;
    int rho = p / (g.F * r.hop);
    if (rho > g.n_runs - 1) rho = g.n_runs - 1;
    for (int q = rho; q >= 0 && q >= rho - 2; --q) {
        int fe = (q + 1) * g.F;
        if (fe > g.n_frames) fe = g.n_frames;
        const int j = p - fe * r.hop;
        if (j >= 0 && j < g.tail_len) {
            const float *t = r.tails + ((size_t)b * g.n_runs + q) * C * g.tail_len;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += t[c * g.tail_len + j];
        }
    }
}
// fn(p) for the padded (centre = N / 2, reflect) positions that sample n of a T-sample clip maps to: the direct one and up to two
// reflected ones
template <typename Fn>
__device__ __forceinline__ void for_padded_positions(int n, int N, int T, Fn &&fn)
{
    fn(n + N / 2);
    if (n >= 1 && n <= N / 2) fn(N / 2 - n);
    if (n <= T - 2 && n >= T - 1 - N / 2) fn(N / 2 + 2 * (T - 1) - n);
}

// ---- partial sums ---------------------------------------------------------------------------------------------------------------
// the workgroup's K fp64 sums -> part[(b * gridDim.x + blockIdx.x) * K + k], fixed order (lanes by butterfly, then the WAVES
// wavefronts); red: WAVES * K doubles of LDS
template <int K, int WAVES>
__device__ __forceinline__ void block_partials(const double (&s)[K], double *red, int b, double *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum_f64(s[k]);
        if (lane == 0) red[wave * K + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double acc = 0.0;
        for (int w = 0; w < WAVES; ++w) acc += red[w * K + threadIdx.x];
        part[((size_t)b * gridDim.x + blockIdx.x) * K + threadIdx.x] = acc;
    }
}
