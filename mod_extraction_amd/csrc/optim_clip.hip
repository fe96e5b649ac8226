// optim_clip.hip -- K12 with gradient clipping: the squared 2-norm of the flat fp32 gradient and the AdamW step of optim.hip
// with the clip folded into the gradient scale (reference: the `gradient_clip_val` / `gradient_clip_algorithm` keys of the
// Lightning trainer section, i.e. torch.nn.utils.clip_grad_norm_ (2-norm, the `+ 1e-6` included) and clip_grad_value_).
// The clip coefficient is formed on the device from the reduced sum, so a clipped optimizer step has no host round trip.
// Both kernels are HBM streaming: 4 B read per parameter for the norm, 16 B read + 12 B written for the update.
#include "common.h"

// ---- mx_grad_sumsq ---------------------------------------------------------------------------------------------------
// Stage 1: workgroup w sums chunks w, w + G, w + 2 G, ... of MX_SUMSQ_CHUNK consecutive elements; thread t of a chunk takes the
// four elements 4 t .. 4 t + 3 of each of its four 1024-element slabs (one 16 B load per lane and slab where the pointer allows
// it), squares them in fp64 (exact: 48 significant bits at most) and adds them in that order.  Lanes by butterfly, then the four
// waves in index order (block256_sum_f64).  Stage 2: thread 0 of one workgroup adds part[0..G) in index order.  Nothing depends
// on the dispatch order, so the same data gives the same bits.  G is mx_sumsq_partials(n) (include/modex_hip.h).
#define MX_SUMSQ_CHUNK 4096
#define MX_SUMSQ_MAX_PARTIALS 1024

static inline long long sumsq_partials(long long n)
{
    const long long g = (n + MX_SUMSQ_CHUNK - 1) / MX_SUMSQ_CHUNK;
    return g < MX_SUMSQ_MAX_PARTIALS ? g : MX_SUMSQ_MAX_PARTIALS;
}

template <bool VEC>
__global__ __launch_bounds__(256) void grad_sumsq_stage1_kernel(const float *__restrict__ g, long long n, long long n_chunks,
                                                                double *__restrict__ part)
{
    __shared__ double red[4];
    double s = 0.0;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long long base = c * MX_SUMSQ_CHUNK;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = base + j * 1024 + (long long)threadIdx.x * 4;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (VEC && i + 3 < n) {
                const float4 q = *reinterpret_cast<const float4 *>(g + i);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i + e < n) v[e] = g[i + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) s += (double)v[e] * (double)v[e];
        }
    }
    const double t = block256_sum_f64(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void grad_sumsq_stage2_kernel(const double *__restrict__ part, int G, double *__restrict__ stat)
{
    __shared__ double sh[MX_SUMSQ_MAX_PARTIALS];
    for (int i = threadIdx.x; i < G; i += 256) sh[i] = part[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < G; ++i) t += sh[i];
        stat[0] = t;
    }
}

MX_EXPORT int mx_grad_sumsq(const float *grad, int64_t n, double *part, double *stat, void *stream)
{
    if (!grad || !part || !stat || n <= 0) return MX_ERR_ARG;
    const long long n_chunks = ((long long)n + MX_SUMSQ_CHUNK - 1) / MX_SUMSQ_CHUNK;
    const int G = (int)sumsq_partials((long long)n);
    if ((reinterpret_cast<uintptr_t>(grad) & 15) == 0)
        hipLaunchKernelGGL(grad_sumsq_stage1_kernel<true>, dim3(G), dim3(256), 0, (hipStream_t)stream, grad, (long long)n, n_chunks,
                           part);
    else
        hipLaunchKernelGGL(grad_sumsq_stage1_kernel<false>, dim3(G), dim3(256), 0, (hipStream_t)stream, grad, (long long)n, n_chunks,
                           part);
    if (mx_launch_status() != MX_OK) return MX_ERR_LAUNCH;
    hipLaunchKernelGGL(grad_sumsq_stage2_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, G, stat);
    return mx_launch_status();
}

// ---- mx_adamw_step_clip ----------------------------------------------------------------------------------------------
// adamw_kernel of optim.hip (same fp32 operations in the same order) except for how gi is formed.  MODE 1: every thread forms
// the same scale s from stat[0] (three fp64 operations and one rounding to fp32; correctly rounded sqrt / divide, so the host
// can restate it exactly).  MODE 2: comparisons, not fminf / fmaxf, so that a NaN gradient stays a NaN as under torch.clamp.
#define MX_CLIP_NORM 1
#define MX_CLIP_VALUE 2

template <int MODE>
__global__ __launch_bounds__(256) void adamw_clip_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                         float *__restrict__ v, long long n, float lr, float beta1, float beta2,
                                                         float eps, float wd, float bias_c1, float bias_c2_sqrt, float grad_scale,
                                                         float clip_val, double *__restrict__ stat)
{
    float s = grad_scale;
    if (MODE == MX_CLIP_NORM) {
        const double norm = sqrt(stat[0]) * (double)grad_scale;
        const double q = (double)clip_val / (norm + 1e-6);
        const double coef = q > 1.0 ? 1.0 : q;                 // torch.clamp(max=1.0): a NaN norm stays a NaN
        s = (float)((double)grad_scale * coef);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) stat[1] = (double)s;
    const float step_size = lr / bias_c1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float gi;
        if (MODE == MX_CLIP_NORM) {
            gi = g[i] * s;
        } else {
            const float t = g[i] * grad_scale;
            gi = t > clip_val ? clip_val : (t < -clip_val ? -clip_val : t);
        }
        float pi = p[i] * (1.0f - lr * wd);                    // param.mul_(1 - lr * weight_decay)
        const float mi = m[i] + (gi - m[i]) * (1.0f - beta1);  // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * beta2 + (1.0f - beta2) * gi * gi;
        const float denom = sqrtf(vi) / bias_c2_sqrt + eps;
        pi -= step_size * (mi / denom);                        // param.addcdiv_(exp_avg, denom, value=-step_size)
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
}

MX_EXPORT int mx_adamw_step_clip(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 int32_t clip_mode, float clip_val, double *stat, void *stream)
{
    if (!param || !grad || !exp_avg || !exp_avg_sq || !stat || n <= 0 || step <= 0) return MX_ERR_ARG;
    if (clip_mode != MX_CLIP_NORM && clip_mode != MX_CLIP_VALUE) return MX_ERR_ARG;
    if (!(clip_val > 0.0f) || std::isinf(clip_val)) return MX_ERR_ARG;       // NaN fails the first comparison
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    int blocks = (int)((n + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (clip_mode == MX_CLIP_NORM)
        hipLaunchKernelGGL(adamw_clip_kernel<MX_CLIP_NORM>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_avg_sq, (long long)n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale,
                           clip_val, stat);
    else
        hipLaunchKernelGGL(adamw_clip_kernel<MX_CLIP_VALUE>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_avg_sq, (long long)n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale,
                           clip_val, stat);
    return mx_launch_status();
}
