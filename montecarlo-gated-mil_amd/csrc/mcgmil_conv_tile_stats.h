// The BatchNorm statistics epilogue (STATS) shared by the fp32 convolution kernels
// (mcgmil_conv32.hip, mcgmil_conv32x3.hip): both hold a wave's 64 x 64 output block as 4 x 4
// accumulator tiles in the 16 x 16 MFMA C layout, which is the same for the fp32 and the bf16
// instructions.
#pragma once
#include <hip/hip_runtime.h>

#include "mcgmil_device.h"

namespace mcgmil {

// Lane 15 of every row of 16 lanes gets the row's sum (DPP row_shr 1, 2, 4, 8: four VALU adds,
// no LDS traffic); the other lanes hold partial sums.
__device__ __forceinline__ float row_sum16(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xF, 0xF, true));
    return v;
}

// The tile's statistics: one (count, mean, M2) block per channel of a BN_CO-channel tile whose
// pixels are shared by WPX waves. acc[i][j]: channels 16 i + 4 kl + v of the wave's 64, pixels
// 16 j + cl; the wave's first nval pixels are valid. Per channel the 16 lanes sum x - sh and
// (x - sh)^2 around sh = the channel's output at the wave's first pixel (lane 16 kl, j = 0),
// row_sum16 adds the lanes, and lane 16 kl + 15 turns the sums into the wave's (count, mean, M2);
// the waves sharing the channels are merged by chan_merge. One channel quad i at a time, so few
// registers are live beside the accumulators, and no division per lane. red: WPX * 3 * BN_CO
// floats of LDS that nothing else uses any more.
template <int BN_CO, int WPX>
__device__ __forceinline__ void tile_stats(const f32x4 (&acc)[4][4], int nval, int wco, int wpx, int lane,
                                           float* red, float* stats, long long row, int Cout, int co0) {
    const int kl = lane >> 4, cl = lane & 15;
    const float n = (float)nval, rn = nval > 0 ? 1.f / n : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float sh[4], S[4], Q[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            sh[v] = __shfl(acc[i][0][v], kl * 16, 64);
            float sum = 0.f, sq = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = 16 * j + cl < nval ? acc[i][j][v] - sh[v] : 0.f;
                sum += d;
                sq = fmaf(d, d, sq);
            }
            S[v] = sum;
            Q[v] = sq;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            S[v] = row_sum16(S[v]);
            Q[v] = row_sum16(Q[v]);
        }
        if (cl == 15) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int local = wco * 64 + 16 * i + 4 * kl + v;
                red[(wpx * 3 + 0) * BN_CO + local] = n;
                red[(wpx * 3 + 1) * BN_CO + local] = nval > 0 ? fmaf(S[v], rn, sh[v]) : 0.f;
                red[(wpx * 3 + 2) * BN_CO + local] = nval > 0 ? fmaxf(Q[v] - S[v] * S[v] * rn, 0.f) : 0.f;
            }
        }
    }
    __syncthreads();
    for (int local = threadIdx.x; local < BN_CO; local += 256) {
        float cn = red[local], cm[1] = {red[BN_CO + local]}, cM2[1] = {red[2 * BN_CO + local]};
        for (int w = 1; w < WPX; ++w) {
            const float mb[1] = {red[(w * 3 + 1) * BN_CO + local]}, M2b[1] = {red[(w * 3 + 2) * BN_CO + local]};
            chan_merge<1>(cn, cm, cM2, red[(w * 3) * BN_CO + local], mb, M2b);
        }
        stats[((size_t)row * 3 + 0) * Cout + co0 + local] = cn;
        stats[((size_t)row * 3 + 1) * Cout + co0 + local] = cm[0];
        stats[((size_t)row * 3 + 2) * Cout + co0 + local] = cM2[0];
    }
}

}  // namespace mcgmil
