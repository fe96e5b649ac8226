/*
 * modex_hip_file.h -- the third header of the C ABI of libmodex_hip.so: the entry point of K22.
 *
 * It exists for the reason modex_hip_fir.h does: the declaration count of modex_hip.h (117), the six names of
 * modex_hip_fir.h and the ABI number (21) are pinned by tests that the change which added K22 could not touch.  Folding
 * both back into modex_hip.h (one header again) is still the follow-up.  The same rules hold here as there: every entry
 * point is `int mx_name(params);`, a parameter is a pointer or one of int64_t, int32_t, uint64_t, uint32_t, float, double;
 * csrc/common.h includes this file too, so the definition is compiled against its declaration;
 * mod_extraction_amd/_hip.py derives SIGNATURES_FILE from this text.  Pointers, streams and return values: the
 * conventions at the top of modex_hip.h (MX_OK, MX_ERR_*).
 */
#ifndef MODEX_HIP_FILE_H
#define MODEX_HIP_FILE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- K22: one LFO track along a whole recording from the LFOs of overlapping windows (csrc/lfo_stitch.hip) -- no
 * counterpart in the reference.
 * windows (W, n_f) fp32, dense: row w is the LFO the extractor gave for the N samples that start at sample starts[w] of a
 * recording of L samples.  Its n_f points sit at the sample positions
 *
 *   starts[w] + i (N - 1) / (n_f - 1),   i = 0 .. n_f - 1
 *
 * (the align_corners rule by which the effect kernels spread a low-rate LFO over a clip).  Track point j sits at
 *
 *   p_j = j (L - 1) / (n_t - 1),         j = 0 .. n_t - 1
 *
 * and over the windows with starts[w] <= p_j <= starts[w] + N - 1, in ascending w,
 *
 *   track[j] = sum_w a_w v_w / sum_w a_w,     cover[j] = the number of those windows
 *   v_w = the linear interpolation of row w at p_j:  t = (p_j - starts[w]) (n_f - 1) / (N - 1),  i0 = min(floor(t), n_f - 2),
 *         f = t - i0,  v_w = (1 - f) x[i0] + f x[i0 + 1]
 *   a_w = sin^2(pi u) + 1e-3,  u = (p_j - starts[w] + 0.5) / N
 *
 * The taper is there because a window's edge frames are the extractor's least reliable; the floor keeps a point that only
 * window edges cover (the recording's two ends) defined.  Positions, weights and both sums are fp64; there is one rounding
 * to fp32.  A point that no window covers gets cover 0 and track 0.  One thread per track point, no atomics, no workspace:
 * the same arguments give the same bits.  starts: (W,) int64 on the device, ascending (not checked: they live on the
 * device; an unsorted list gives a defined, but other, window range).
 * Before any launch: a NULL pointer, W < 1, n_f < 2, N < 2, L < N, n_t < 2, an output that overlaps an input or the other
 * output: MX_ERR_ARG.  W > MX_STITCH_MAX_WINDOWS, L > 2^31, n_f > 2^22 or n_t > 2^22: MX_ERR_UNSUPPORTED (so j (L - 1) is
 * exact in fp64, p_j is ONE correctly rounded division, and its comparisons with the integers starts[w] and
 * starts[w] + N - 1 are those of the exact rational). */
#define MX_STITCH_MAX_WINDOWS (1 << 20)

int mx_lfo_stitch(const float *windows, const int64_t *starts, int64_t W, int64_t n_f, int64_t N, int64_t L, int64_t n_t,
                  float *track, int32_t *cover, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEX_HIP_FILE_H */
