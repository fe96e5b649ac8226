// phaser_common.h -- what the phaser scan (phaser.hip) and its adjoint (phaser_bwd.hip) share: the chunking of a clip and the
// layout of the stash that mx_phaser_fwd_stash leaves for mx_phaser_bwd.
#pragma once
#include "common.h"

#define PS_WAVES 8
#define PS_P (64 * PS_WAVES)       // chunks (lanes) per clip
#define PS_MV 57                   // floats per chunk map: M column-major (49) + v (7) + pad
#define PS_LDS_FLOATS (PS_P * PS_MV + (PS_P + 1) * 8)
#define PS_SUB 2                   // cut-off groups (of 4 samples) between two state checkpoints of the stash (a power of two)

// Stash row of one clip, `sg` = stash_groups (a multiple of 4, >= the clip's cut-off groups), in floats:
//   [0, sg) G   [sg, 2 sg) pre = osc depth / 2 + norm_centre (before its clamp)   [2 sg, 3 sg) osc
//   [3 sg, 4 sg) int32: bit j set where sample 4 g + j passed the output clip (-1 <= m <= 1)
//   then PS_P chunk maps of PS_MV floats (the scan's M, column-major, + v), then the state checkpoints: 8 floats
//   (s0..s5, lastOut, pad) at the start of every PS_SUB-th group of every chunk, chunk p's at (p * spc + i) * 8 with
//   spc = ceil(groups per chunk / PS_SUB) of THAT clip.
__host__ __device__ inline long long ps_ckpts_per_chunk(long long n_groups)
{
    const long long gpc = (n_groups + PS_P - 1) / PS_P;
    return (gpc + PS_SUB - 1) / PS_SUB;
}
__host__ __device__ inline long long ps_stash_floats(long long sg)
{
    return 4 * sg + (long long)PS_P * PS_MV + (long long)PS_P * 8 * ps_ckpts_per_chunk(sg);
}
