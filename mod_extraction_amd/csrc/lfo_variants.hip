// lfo_variants.hip -- K14: the evaluation LFO variants for a whole batch (reference: mod_extraction/modulations.py:104-160
// make_quasi_periodic, :191-210 make_combined_mod_sig, as datasets.py:365-398 applies them to every item).
//
// The reference walks one LFO at a time on the host: corner indices are pulled out of a tensor, and every corner-to-corner
// section costs a random draw and a resampling / synthesis call.  Here the random numbers come in as a FIXED-WIDTH table per
// row (S entries, drawn by the host before the launch) and the code that knows the corners consumes them in order, so one
// launch serves the batch and nothing returns to the host.
//
// One 256-thread workgroup per row, two passes:
//   1. the row is swept in index order, 256 points at a time; every point evaluates the corner rule of find_corners
//      (corner_values) and the corners are appended IN ORDER to a short LDS list (wave ballot + prefix over the four waves);
//   2. thread 0 turns the list into a section table (at most S + 1 entries); every output point then finds its section by a
//      scan of that table and evaluates either the two taps of the align_corners resampling (interp_tap / interp_combine)
//      or the closed-form LFO value (lfo_value) -- the very device functions the per-item path runs, hence the same bits.
// LDS holds the corner lists and the section table only (under 2 KB), the rows stay in global memory: the row length is
// bounded by the fp32 index arithmetic of interp_tap (exact below 2^24), not by LDS.  No atomics, no workspace, fixed
// order everywhere: results are identical from run to run.  ~3.5 KB per 882-point row: bookkeeping, not a roofline target.
#include "lfo_common.h"

#define LV_THREADS 256
#define LV_MAX_S 64
#define LV_MAX_N (1ll << 24)

// Appends `value` of every thread whose `flag` is set to list[0 .. cap), in thread order, behind the `have` entries of the
// earlier sweeps; returns the new count (which keeps counting beyond cap).  Called by all LV_THREADS threads; cnt: 4 ints.
__device__ __forceinline__ int append_in_order(bool flag, int value, int *list, int cap, int have, int *cnt)
{
    const unsigned long long mask = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();                                            // cnt may still be read from the previous call
    if (lane == 0) cnt[w] = __popcll(mask);
    __syncthreads();
    int at = have;
    for (int q = 0; q < w; ++q) at += cnt[q];
    if (flag && at + before < cap) list[at + before] = value;
    return have + cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// ---- make_quasi_periodic (modulations.py:104-160) ----------------------------------------------------------------
__global__ __launch_bounds__(LV_THREADS) void lfo_quasi_periodic_kernel(const float *__restrict__ base,
                                                                        const int *__restrict__ shrink,
                                                                        const float *__restrict__ amount, int n, int S,
                                                                        float *__restrict__ out,
                                                                        int *__restrict__ n_corners)
{
    __shared__ int top_at[LV_MAX_S], bot_at[LV_MAX_S];
    __shared__ int cnt[2][4];
    __shared__ double red[4];
    // section s < m: base[src .. src + n_in) resampled to n_out points, the first n_out - 1 of them from output index off;
    // section m: the tail.  off[m + 1] = n closes the table.
    __shared__ int sec_src[LV_MAX_S + 1], sec_in[LV_MAX_S + 1], sec_out[LV_MAX_S + 1], sec_off[LV_MAX_S + 2];

    const int b = blockIdx.x, tid = threadIdx.x;
    const float *m = base + (size_t)b * n;
    float *o = out + (size_t)b * n;

    // pass 1: both corner maps (modulations.py:128), their sums and the ordered index lists of the entries equal to 1
    int n_top = 0, n_bot = 0;
    double sum_top = 0.0, sum_bot = 0.0;                        // the maps hold integers: exact in any order
    for (int c0 = 0; c0 < n; c0 += LV_THREADS) {
        const int i = c0 + tid;
        float t = 0.0f, bt = 0.0f;
        if (i >= 1 && i <= n - 2) corner_values(m, i, t, bt);
        sum_top += (double)t;
        sum_bot += (double)bt;
        n_top = append_in_order(t == 1.0f, i, top_at, S, n_top, cnt[0]);
        n_bot = append_in_order(bt == 1.0f, i, bot_at, S, n_bot, cnt[1]);
    }
    sum_top = block256_sum_f64(sum_top, red);
    sum_bot = block256_sum_f64(sum_bot, red);
    const bool use_top = sum_top > sum_bot;                     // modulations.py:129-132
    const int *at = use_top ? top_at : bot_at;
    const int mc = use_top ? n_top : n_bot;
    if (tid == 0 && n_corners) n_corners[b] = mc;
    if (mc < 2 || mc > S) {                                     // modulations.py:136-137; more corners than table entries
        for (int j = tid; j < n; j += LV_THREADS) o[j] = m[j];
        return;
    }

    // the section table (modulations.py:139-156 with _time_stretch_section, :104-118): serial, at most S entries
    if (tid == 0) {
        long long off = 0;
        int prev = 0;
        for (int s = 0; s < mc; ++s) {
            const int c = at[s];
            const int size = c - prev + 1;
            double xd = (double)amount[(size_t)b * S + s] * (double)size + 0.5;
            xd = fmin(fmax(xd, -1073741824.0), 1073741824.0);  // keeps the conversion defined for a table of nonsense
            const long long x = (long long)xd;                  // int(): towards zero
            long long nw = shrink[(size_t)b * S + s] ? (long long)size - x : (long long)size + x;
            nw = nw < 2 ? 2 : nw;
            sec_src[s] = prev;
            sec_in[s] = size;
            sec_out[s] = (int)nw;
            sec_off[s] = (int)(off < n ? off : n);
            off += nw - 1;                                      // new_section[:-1]
            prev = c;
        }
        const int tail = n - prev;
        const long long total = off + tail;
        sec_src[mc] = prev;
        sec_in[mc] = tail;
        sec_out[mc] = total < n ? tail + (int)(n - total) : tail;   // modulations.py:153-155
        sec_off[mc] = (int)(off < n ? off : n);
        sec_off[mc + 1] = n;
    }
    __syncthreads();

    // pass 2: one thread per output point of torch.cat(sections)[:n]
    for (int j = tid; j < n; j += LV_THREADS) {
        int s = 0;
        while (s < mc && sec_off[s + 1] <= j) ++s;
        const int k = j - sec_off[s];
        const int n_in = sec_in[s], n_out = sec_out[s];
        const float *src = m + sec_src[s];
        float v;
        if (n_in == n_out) {                                    // util.py:15-29 returns its input
            v = src[k];
        } else {
            const float scale = __fdiv_rn((float)(n_in - 1), (float)(n_out - 1));
            const InterpTap t = interp_tap(scale, k, n_in);
            v = interp_combine(t, src[t.i0], src[t.i1]);
        }
        o[j] = v;
    }
}

MX_EXPORT int mx_lfo_quasi_periodic(const float *base, const int32_t *shrink, const float *amount, int64_t B, int64_t n,
                                    int64_t S, float *out, int32_t *n_corners, void *stream)
{
    if (!base || !shrink || !amount || !out || out == base || B <= 0 || n < 3 || S < 0) return MX_ERR_ARG;
    if (S < 1 || S > LV_MAX_S || n > LV_MAX_N || B > 0x7fffffffll) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lfo_quasi_periodic_kernel, dim3((unsigned)B), dim3(LV_THREADS), 0, (hipStream_t)stream, base,
                       shrink, amount, (int)n, (int)S, out, n_corners);
    return mx_launch_status();
}

// ---- make_combined_mod_sig (modulations.py:191-210) ------------------------------------------------------------------
__global__ __launch_bounds__(LV_THREADS) void lfo_combined_kernel(const float *__restrict__ freq,
                                                                  const float *__restrict__ phase,
                                                                  const int *__restrict__ shape_tab, int n, int S,
                                                                  float sr, float *__restrict__ out,
                                                                  int *__restrict__ n_corners)
{
    __shared__ int bot_at[LV_MAX_S + 1];                        // S pairs need S + 1 corners
    __shared__ int cnt[4];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int *tab = shape_tab + (size_t)b * (S + 1);
    float *o = out + (size_t)b * n;

    // pass 1: the base LFO (lfo_synth_kernel with exponent 1 and start 0) and its bottom corners
    const int sh0 = tab[0];
    float f = freq[b], ph = phase[b];
    const float step = lfo_step(sh0, f, ph, sr);
    int mc = 0;
    for (int c0 = 0; c0 < n; c0 += LV_THREADS) {
        const int i = c0 + tid;
        bool is_bot = false;
        if (i < n) {
            float w[3];
            w[1] = lfo_value(i, 0, step, ph, sh0, 1.0f);
            if (i >= 1 && i <= n - 2) {
                float t, bt;
                w[0] = lfo_value(i - 1, 0, step, ph, sh0, 1.0f);
                w[2] = lfo_value(i + 1, 0, step, ph, sh0, 1.0f);
                corner_values(w, 1, t, bt);
                is_bot = bt == 1.0f;
            }
            o[i] = w[1];
        }
        mc = append_in_order(is_bot, i, bot_at, S + 1, mc, cnt);
    }
    if (tid == 0 && n_corners) n_corners[b] = mc;
    if (mc < 2) return;                                         // modulations.py:203
    __syncthreads();

    // pass 2: points c_s .. c_(s+1) take a fresh LFO of one period over the section (modulations.py:204-209); a shared
    // corner belongs to the later section (the later assignment of the reference's loop wins), the last corner to the last
    // section.  Every thread rewrites only points it wrote in pass 1.
    const int listed = mc < S + 1 ? mc : S + 1;
    for (int j = tid; j < n; j += LV_THREADS) {
        if (j < bot_at[0] || j > bot_at[listed - 1]) continue;
        int seen = 0;
        while (seen < listed && bot_at[seen] <= j) ++seen;
        int s = seen - 1;
        if (seen == mc) s = mc - 2;
        if (s >= S) continue;                                   // pairs beyond the table keep the base
        const int a = bot_at[s];
        const int sh = tab[s + 1];
        float f1 = 1.0f, ph1 = 0.0f;
        const float step1 = lfo_step(sh, f1, ph1, (float)(bot_at[s + 1] - a + 1));
        o[j] = lfo_value(j - a, 0, step1, ph1, sh, 1.0f);
    }
}

MX_EXPORT int mx_lfo_combined(const float *freq, const float *phase, const int32_t *shape_tab, int64_t B, int64_t n,
                              int64_t S, float sr, float *out, int32_t *n_corners, void *stream)
{
    if (!freq || !phase || !shape_tab || !out || B <= 0 || n <= 0 || S < 0 || !(sr > 0.0f)) return MX_ERR_ARG;
    if (S < 1 || S > LV_MAX_S || n > LV_MAX_N || B > 0x7fffffffll) return MX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lfo_combined_kernel, dim3((unsigned)B), dim3(LV_THREADS), 0, (hipStream_t)stream, freq, phase,
                       shape_tab, (int)n, (int)S, sr, out, n_corners);
    return mx_launch_status();
}
