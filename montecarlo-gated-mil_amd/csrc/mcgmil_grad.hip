// Backward pass of the MCDO gated-attention MIL head (include/mcgmil_grad.h) for gfx950, fp32.
//
// Forward (mcgmil_kernels.h), one bag, sample t, class c, gate g = c (separate) or 0 (shared):
//   X = H (.) keepF        Hd = X sf        V = tanh(Hd Wv_g^T + bv_g)   U = sigmoid(Hd Wu_g^T + bu_g)
//   z_c = ((V (.) U) wa_c + ba_c) (.) keepA_c sa     A_c = softmax_n z_c     Y_c = (A_c^T Hd) wk_c
// Backward, from dY, an optional dA and the saved A, Y (no mask is stored: keepF / keepA are drawn
// again from the forward's Philox counters):
//   q_c = Hd wk_c     dz_c = A_c (dY_c q_c + dA_c - r_c),  r_c = dY_c Y_c + sum_m A_c dA_c
//   ds_c = dz_c (.) keepA_c sa     dG = sum_{c on g} ds_c wa_c
//   dPv = dG U (1 - V^2)           dPu = dG V U (1 - U)
//   dHd = dPv Wv_g + dPu Wu_g + sum_c A_c dY_c wk_c         dH = sum_t dHd (.) keepF sf
//   dWv_g = dPv^T Hd, dWu_g = dPu^T Hd, dwk_c = (A_c dY_c)^T Hd, dbv = sum dPv, dbu = sum dPu,
//   dwa_c = ds_c^T (V (.) U), dba_c = sum ds_c, all summed over t and bags.
//
// Kernels (three MFMA GEMMs on v_mfma_f32_16x16x4_f32 through Frag<float> / mma):
//   grad_rows_kernel    a workgroup owns a tile of 32 (or 16) rows of H and loops over the T samples:
//                       masked tile -> LDS, q and the gate GEMM again, the epilogue above, dP = [dPv |
//                       dPu | A dY] -> LDS and workspace, the dHd GEMM, dH (each row is owned by one
//                       workgroup: plain read-add-write over t, no atomics), and the tile's partial
//                       dbv / dbu / dwa / dba -> workspace.
//   grad_weights_kernel [dWv ; dWu ; dwk] = dP^T Hd, split along K into granules of
//                       MCGMIL_GRAD_GRANULE_ROWS rows of H (all their T samples): one partial per
//                       granule -> workspace. Hd is rebuilt from H and Philox.
//   grad_reduce_kernel  sums the partials strictly in row order into the outputs (or, between
//                       launch chunks, into accumulators): the order is the same however the
//                       launcher chunks the call, so the result is bitwise the same.
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/mcgmil_grad.h"
#include "mcgmil_device.h"
#include "mcgmil_error.h"

namespace mcgmil {

constexpr int kGradThreads = 512;       // grad_rows_kernel: 8 waves
constexpr int kGradWaves = kGradThreads / kWave;
constexpr int kGradPPW = 2;             // gate tile pairs per wave and pass
constexpr int kGradPad = 4;             // floats of padding per dP row in LDS (conflict-free b128 reads)
constexpr int kGradRowInfo = 6;         // valid, bag, n, Nb, bag counter, A base (low 32 bits unused)
constexpr int kWThreads = 256;          // grad_weights_kernel: 4 waves, 64 x 64 outputs
constexpr int kWStride = 68;            // floats per staged row (64 + pad, 16-byte multiple)
constexpr int kGranule = MCGMIL_GRAD_GRANULE_ROWS;

struct GradParams {
    const float* H;
    long long ldh;
    const int32_t* bag_off;
    const uint32_t* bag_ids;
    uint32_t bag_base;
    int t_base;
    int B, T, L, D, C, G;
    int J, K2, Kw;                 // J = G*D, K2 = 2J gate columns, Kw = K2 + 16 columns of dP
    const float *Wv, *Wu, *bv, *bu, *wa, *wk;
    const float* WT;               // [L][K2]: column k of row l = Wv / Wu row k, feature l
    const float *A, *Y, *dY, *dA, *rA;
    float sf, sa;
    uint32_t thr_f, thr_a, k0, k1;
    long long row0;                // first row of H of this launch chunk
    int rows;                      // its rows
    int Rc;                        // rows per sample in the dP workspace (row stride of t)
    int2* rowinfo;                 // [Rc] (n, bag counter) of the chunk's rows
    float* dP;                     // [T][Rc][Kw]
    float* partA;                  // [row tiles][NPA]
    int NPA;                       // C*D (dwa) + J (dbv) + J (dbu) + C (dba)
    float* partB;                  // [granules][Kw][L]
    float* dH;
    long long lddh;
};

__host__ __device__ constexpr size_t grad_rows_lds_bytes(int BM, int L, int K2, int NPA) {
    return ((size_t)BM * L + (size_t)BM * (K2 + kGradPad) + 3 * 4 * (size_t)BM + (size_t)((NPA + 3) & ~3)) * 4 +
           (size_t)BM * kGradRowInfo * 4 + (size_t)BM * (L / 8);
}

// sum_m A dA per (bag, t, c), in a fixed order: strided per-thread sums, the wave butterfly, then
// the four wave sums in wave order.
__global__ __launch_bounds__(256) void grad_ra_kernel(const int32_t* bag_off, int T, int C, const float* A,
                                                      const float* dA, float* rA) {
    __shared__ float part[4];
    const int b = blockIdx.x, tc = blockIdx.y;
    const int ob = bag_off[b], Nb = bag_off[b + 1] - ob;
    const size_t base = (size_t)T * C * ob + (size_t)tc * Nb;
    float s = 0.f;
    for (int n = threadIdx.x; n < Nb; n += 256) s = fmaf(A[base + n], dA[base + n], s);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) rA[(size_t)b * T * C + tc] = ((part[0] + part[1]) + part[2]) + part[3];
}

// WT[l][k] = Wv[k][l] (k < J) or Wu[k - J][l]: the dHd GEMM's A operand, K-contiguous per feature.
__global__ void grad_pack_kernel(const float* Wv, const float* Wu, int L, int J, float* WT) {
    const size_t total = (size_t)L * 2 * J;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(i / (2 * J)), k = (int)(i - (size_t)l * 2 * J);
        WT[i] = k < J ? Wv[(size_t)k * L + l] : Wu[(size_t)(k - J) * L + l];
    }
}

template <int RT>
__global__ __launch_bounds__(kGradThreads) void grad_rows_kernel(const GradParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BM = 16 * RT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = p.L, KS = L >> 5, LC = L >> 3, SP = p.K2 + kGradPad;
    const int DB = p.D >> 4, P = p.G * DB;

    float* Xs = reinterpret_cast<float*>(smem);
    float* dPs = Xs + (size_t)BM * L;
    float* qs = dPs + (size_t)BM * SP;
    float* dss = qs + 4 * BM;
    float* acs = dss + 4 * BM;
    float* pacc = acs + 4 * BM;
    int* rinfo = reinterpret_cast<int*>(pacc + ((p.NPA + 3) & ~3));
    uint8_t* keepb = reinterpret_cast<uint8_t*>(rinfo + BM * kGradRowInfo);
    const int o_dbv = p.C * p.D, o_dbu = o_dbv + p.J, o_dba = o_dbu + p.J;

    const int tile = blockIdx.x;
    const int lr0 = tile * BM;                       // chunk-local first row
    if (tid < BM) {
        const int lr = lr0 + tid;
        int valid = lr < p.rows, bag = 0, n = 0, Nb = 1, bagc = 0;
        if (valid) {
            const long long hrow = p.row0 + lr;
            bag = find_bag(p.bag_off, p.B, 1, hrow);
            const int ob = p.bag_off[bag];
            Nb = p.bag_off[bag + 1] - ob;
            n = (int)(hrow - ob);
            bagc = (int)(p.bag_ids ? p.bag_ids[bag] : p.bag_base + (uint32_t)bag);
            p.rowinfo[lr] = make_int2(n, bagc);
        }
        int* ri = rinfo + kGradRowInfo * tid;
        ri[0] = valid; ri[1] = bag; ri[2] = n; ri[3] = Nb; ri[4] = bagc; ri[5] = 0;
    }
    for (int i = tid; i < p.NPA; i += kGradThreads) pacc[i] = 0.f;
    __syncthreads();

    for (int t = 0; t < p.T; ++t) {
        // ---- masked feature tile (fragment layout of gate_scores_kernel) + its keep bytes ----
        for (int i = tid; i < BM * LC; i += kGradThreads) {
            const int blk = i >> 6, slot = i & 63;
            const int rt = blk / KS, ks = blk - rt * KS;
            const int r = rt * 16 + (slot & 15);
            const int kc = ks * 4 + (slot >> 4);
            float* dst = Xs + ((size_t)blk * 64 + slot) * 8;
            const int* ri = rinfo + kGradRowInfo * r;
            if (!ri[0]) {
                store_zero8(dst);
                keepb[r * LC + kc] = 0;
                continue;
            }
            const uint4 o = philox4x32_10((uint32_t)kc, (uint32_t)ri[2], (uint32_t)(p.t_base + t),
                                          (uint32_t)ri[4], p.k0, p.k1);
            const uint32_t kb = keep_byte(o, p.thr_f);
            keepb[r * LC + kc] = (uint8_t)kb;
            load_masked(p.H + (size_t)(p.row0 + lr0 + r) * p.ldh + (size_t)kc * 8, kb, dst);
        }
        __syncthreads();

        // ---- q_c[n] = sf X[n] . wk_c (the forward's classifier projection, same MFMA order) ----
        if (wave < RT) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int c = lane & 15;
            for (int ks = 0; ks < KS; ++ks) {
                const Frag<float> a = c < p.C ? load_frag(p.wk + (size_t)c * L + ks * 32 + 8 * (lane >> 4))
                                              : zero_frag<float>();
                const Frag<float> x = load_frag(Xs + ((size_t)(wave * KS + ks) * 64 + lane) * 8);
                acc = mma(a, x, acc);
            }
            if (lane < 16) {
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) qs[c4 * BM + wave * 16 + lane] = acc[c4] * p.sf;
            }
        }
        __syncthreads();

        // ---- ds_c[n] and the pooling coefficient A_c[n] dY_c ----
        if (tid < 4 * BM) {
            const int c = tid / BM, r = tid - c * BM;
            const int* ri = rinfo + kGradRowInfo * r;
            float ds = 0.f, ac = 0.f;
            if (c < p.C && ri[0]) {
                const int bag = ri[1], n = ri[2], Nb = ri[3];
                const size_t ai = (size_t)p.T * p.C * (size_t)p.bag_off[bag] + ((size_t)t * p.C + c) * Nb + n;
                const size_t yi = ((size_t)bag * p.T + t) * p.C + c;
                const float Av = p.A[ai], dy = p.dY[yi], yv = p.Y[yi];
                const float da = p.dA ? p.dA[ai] : 0.f, ra = p.rA ? p.rA[yi] : 0.f;
                // both sides in the same form: for a one-instance bag (q = Y, dA = rA) dz is exactly 0
                const float dat = __fmaf_rn(dy, qs[c * BM + r], da);
                const float rr = __fmaf_rn(dy, yv, ra);
                const float dz = Av * (dat - rr);
                const bool keep = attention_keep(p.k0, p.k1, (uint32_t)ri[4], (uint32_t)(p.t_base + t),
                                                 (uint32_t)c, (uint32_t)n, p.thr_a);
                ds = keep ? dz * p.sa : 0.f;
                ac = Av * dy;
            }
            dss[tid] = ds;
            acs[tid] = ac;
        }
        __syncthreads();
        if (tid < p.C) {
            float s = 0.f;
            for (int r = 0; r < BM; ++r) s += dss[tid * BM + r];
            pacc[o_dba + tid] += s;
        }
        if (tid < 4 * BM) {      // columns K2 .. K2+15 of dP: A_c dY_c, then zeros
            const int r = tid >> 2, quad = tid & 3;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (quad == 0) v = f32x4{acs[r], acs[BM + r], acs[2 * BM + r], acs[3 * BM + r]};
            *reinterpret_cast<f32x4*>(p.dP + ((size_t)t * p.Rc + lr0 + r) * p.Kw + p.K2 + 4 * quad) = v;
        }

        // ---- gate GEMM again, the epilogue, dP ----
        const int npass = (P + kGradWaves * kGradPPW - 1) / (kGradWaves * kGradPPW);
        for (int pass = 0; pass < npass; ++pass) {
            const int q0 = (pass * kGradWaves + wave) * kGradPPW;
            if (q0 >= P) continue;
            f32x4 acc[RT][2 * kGradPPW];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int j = 0; j < 2 * kGradPPW; ++j) acc[rt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* wbase[2 * kGradPPW];
#pragma unroll
            for (int j = 0; j < 2 * kGradPPW; ++j) {
                int q = q0 + (j >> 1);
                q = q < P ? q : P - 1;
                const int g = q / DB, db = q - g * DB;
                wbase[j] = ((j & 1) ? p.Wu : p.Wv) + ((size_t)g * p.D + db * 16 + (lane & 15)) * L + 8 * (lane >> 4);
            }
            for (int ks = 0; ks < KS; ++ks) {
                Frag<float> w[2 * kGradPPW];
#pragma unroll
                for (int j = 0; j < 2 * kGradPPW; ++j) w[j] = load_frag(wbase[j] + ks * 32);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const Frag<float> x = load_frag(Xs + ((size_t)(rt * KS + ks) * 64 + lane) * 8);
#pragma unroll
                    for (int j = 0; j < 2 * kGradPPW; ++j) acc[rt][j] = mma(w[j], x, acc[rt][j]);
                }
            }
#pragma unroll
            for (int jp = 0; jp < kGradPPW; ++jp) {
                const int q = q0 + jp;
                if (q >= P) break;
                const int g = q / DB, db = q - g * DB;
                const int d0 = db * 16 + 4 * (lane >> 4);
                const f32x4 bvv = *reinterpret_cast<const f32x4*>(p.bv + (size_t)g * p.D + d0);
                const f32x4 buv = *reinterpret_cast<const f32x4*>(p.bu + (size_t)g * p.D + d0);
                f32x4 wac[4];
                bool use[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    use[c] = c < p.C && (p.G == 1 || c == g);
                    wac[c] = use[c] ? *reinterpret_cast<const f32x4*>(p.wa + (size_t)c * p.D + d0)
                                    : f32x4{0.f, 0.f, 0.f, 0.f};
                }
                f32x4 s_bv = {0.f, 0.f, 0.f, 0.f}, s_bu = s_bv, s_wa[4] = {s_bv, s_bv, s_bv, s_bv};
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int r = rt * 16 + (lane & 15);
                    float dsc[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) dsc[c] = use[c] ? dss[c * BM + r] : 0.f;
                    f32x4 dpv, dpu;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float V = tanhf(fmaf(acc[rt][2 * jp][v], p.sf, bvv[v]));
                        const float U = 1.0f / (1.0f + expf(-fmaf(acc[rt][2 * jp + 1][v], p.sf, buv[v])));
                        const float vu = V * U;
                        float dG = 0.f;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            dG = fmaf(dsc[c], wac[c][v], dG);
                            s_wa[c][v] = fmaf(dsc[c], vu, s_wa[c][v]);
                        }
                        dpv[v] = dG * U * (1.0f - V * V);
                        dpu[v] = dG * vu * (1.0f - U);
                        s_bv[v] += dpv[v];
                        s_bu[v] += dpu[v];
                    }
                    const int col = g * p.D + d0;
                    *reinterpret_cast<f32x4*>(dPs + (size_t)r * SP + col) = dpv;
                    *reinterpret_cast<f32x4*>(dPs + (size_t)r * SP + p.J + col) = dpu;
                    float* gp = p.dP + ((size_t)t * p.Rc + lr0 + r) * p.Kw + col;
                    *reinterpret_cast<f32x4*>(gp) = dpv;
                    *reinterpret_cast<f32x4*>(gp + p.J) = dpu;
                }
                // sums over the tile's rows: the 16 lanes sharing lane >> 4, fixed butterfly order
#pragma unroll
                for (int v = 0; v < 4; ++v) {
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) {
                        s_bv[v] += __shfl_xor(s_bv[v], o);
                        s_bu[v] += __shfl_xor(s_bu[v], o);
#pragma unroll
                        for (int c = 0; c < 4; ++c) s_wa[c][v] += __shfl_xor(s_wa[c][v], o);
                    }
                }
                if ((lane & 15) == 0) {      // this lane alone owns these pacc entries
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        pacc[o_dbv + g * p.D + d0 + v] += s_bv[v];
                        pacc[o_dbu + g * p.D + d0 + v] += s_bu[v];
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (use[c]) pacc[c * p.D + d0 + v] += s_wa[c][v];
                    }
                }
            }
        }
        __syncthreads();

        // ---- dHd = dP [Wv ; Wu] + sum_c (A_c dY_c) wk_c, masked and added into dH ----
        if (p.dH) {
            const int KS2 = p.K2 >> 5;
            for (int ft = wave; ft < (L >> 4); ft += kGradWaves) {
                f32x4 acc[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
                const float* wt = p.WT + (size_t)(ft * 16 + (lane & 15)) * p.K2 + 8 * (lane >> 4);
                for (int ks = 0; ks < KS2; ++ks) {
                    const Frag<float> a = load_frag(wt + ks * 32);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const Frag<float> b = load_frag(dPs + (size_t)(rt * 16 + (lane & 15)) * SP + ks * 32 + 8 * (lane >> 4));
                        acc[rt] = mma(a, b, acc[rt]);
                    }
                }
                const int l0 = ft * 16 + 4 * (lane >> 4);
                f32x4 wkv[4];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    wkv[c] = c < p.C ? *reinterpret_cast<const f32x4*>(p.wk + (size_t)c * L + l0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int r = rt * 16 + (lane & 15);
                    if (!rinfo[kGradRowInfo * r]) continue;
                    const uint32_t kb = (uint32_t)keepb[r * LC + (l0 >> 3)] >> (l0 & 7);
                    f32x4 out;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        float val = acc[rt][v];
#pragma unroll
                        for (int c = 0; c < 4; ++c) val = fmaf(acs[c * BM + r], wkv[c][v], val);
                        out[v] = ((kb >> v) & 1u) ? val * p.sf : 0.f;
                    }
                    f32x4* dst = reinterpret_cast<f32x4*>(p.dH + (size_t)(p.row0 + lr0 + r) * p.lddh + l0);
                    if (t > 0) out += *dst;
                    *dst = out;
                }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < p.NPA; i += kGradThreads) p.partA[(size_t)tile * p.NPA + i] = pacc[i];
}

// One 64 (columns of dP) x 64 (features) tile of dP^T Hd over one granule of rows, all T samples.
__global__ __launch_bounds__(kWThreads) void grad_weights_kernel(const GradParams p) {
    __shared__ __attribute__((aligned(16))) float As[32 * kWStride];
    __shared__ __attribute__((aligned(16))) float Bs[32 * kWStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int gr0 = blockIdx.z * kGranule;
    const int gr1 = gr0 + kGranule < p.rows ? gr0 + kGranule : p.rows;
    const int spt = (gr1 - gr0 + 31) >> 5, steps = spt * p.T;
    const int sr = tid >> 3, oc = tid & 7;             // staging: row, octet of 8 columns
    const bool a_in = c0 + oc * 8 < p.Kw, b_in = f0 + oc * 8 < p.L;
    const int cw = c0 + wave * 16;
    const bool active = cw < p.Kw;

    f32x4 acc[4];
#pragma unroll
    for (int fs = 0; fs < 4; ++fs) acc[fs] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra0, ra1, rb0, rb1;
    uint32_t rkb = 0;

    auto fetch = [&](int step) {
        const int t = step / spt, row = gr0 + ((step - t * spt) << 5) + sr;
        ra0 = ra1 = rb0 = rb1 = f32x4{0.f, 0.f, 0.f, 0.f};
        rkb = 0;
        if (row >= gr1) return;
        if (a_in) {
            const float* src = p.dP + ((size_t)t * p.Rc + row) * p.Kw + c0 + oc * 8;
            ra0 = *reinterpret_cast<const f32x4*>(src);
            ra1 = *reinterpret_cast<const f32x4*>(src + 4);
        }
        if (b_in) {
            const int2 ri = p.rowinfo[row];
            const uint4 o = philox4x32_10((uint32_t)((f0 >> 3) + oc), (uint32_t)ri.x, (uint32_t)(p.t_base + t),
                                          (uint32_t)ri.y, p.k0, p.k1);
            rkb = keep_byte(o, p.thr_f);
            const float* src = p.H + (size_t)(p.row0 + row) * p.ldh + f0 + oc * 8;
            rb0 = *reinterpret_cast<const f32x4*>(src);
            rb1 = *reinterpret_cast<const f32x4*>(src + 4);
        }
    };

    if (steps > 0) fetch(0);
    for (int step = 0; step < steps; ++step) {
        __syncthreads();
        {
            float* da = As + sr * kWStride + oc * 8;
            *reinterpret_cast<f32x4*>(da) = ra0;
            *reinterpret_cast<f32x4*>(da + 4) = ra1;
            f32x4 b0 = rb0, b1 = rb1;
            b0.x = (rkb & 1u) ? b0.x : 0.f;   b0.y = (rkb & 2u) ? b0.y : 0.f;
            b0.z = (rkb & 4u) ? b0.z : 0.f;   b0.w = (rkb & 8u) ? b0.w : 0.f;
            b1.x = (rkb & 16u) ? b1.x : 0.f;  b1.y = (rkb & 32u) ? b1.y : 0.f;
            b1.z = (rkb & 64u) ? b1.z : 0.f;  b1.w = (rkb & 128u) ? b1.w : 0.f;
            float* db = Bs + sr * kWStride + oc * 8;
            *reinterpret_cast<f32x4*>(db) = b0;
            *reinterpret_cast<f32x4*>(db + 4) = b1;
        }
        __syncthreads();
        if (step + 1 < steps) fetch(step + 1);
        if (active) {
            // fragment element j of lane l = staged row 8 (l >> 4) + j, column l & 15
            const float* ap = As + 8 * (lane >> 4) * kWStride + wave * 16 + (lane & 15);
            Frag<float> a;
            a.lo = f32x4{ap[0], ap[kWStride], ap[2 * kWStride], ap[3 * kWStride]};
            a.hi = f32x4{ap[4 * kWStride], ap[5 * kWStride], ap[6 * kWStride], ap[7 * kWStride]};
#pragma unroll
            for (int fs = 0; fs < 4; ++fs) {
                const float* bp = Bs + 8 * (lane >> 4) * kWStride + fs * 16 + (lane & 15);
                Frag<float> b;
                b.lo = f32x4{bp[0], bp[kWStride], bp[2 * kWStride], bp[3 * kWStride]};
                b.hi = f32x4{bp[4 * kWStride], bp[5 * kWStride], bp[6 * kWStride], bp[7 * kWStride]};
                acc[fs] = mma(a, b, acc[fs]);
            }
        }
    }
    if (!active) return;
    float* out = p.partB + (size_t)blockIdx.z * p.Kw * p.L;
#pragma unroll
    for (int fs = 0; fs < 4; ++fs) {
        const int f = f0 + fs * 16 + (lane & 15);
        if (f >= p.L) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(size_t)(cw + 4 * (lane >> 4) + v) * p.L + f] = acc[fs][v] * p.sf;
    }
}

struct ReduceParams {
    const float *partA, *partB;
    float *accA, *accB;
    int ntiles, ngran, NPA, Kw, L, J, C, D;
    int first, last;
    float *dWv, *dbv, *dWu, *dbu, *dwa, *dba, *dwk;
};

// One thread per output element; the partials are added one after the other in row order, on
// top of the accumulator of the chunks before (the same chain of additions for any chunking).
__global__ __launch_bounds__(256) void grad_reduce_kernel(const ReduceParams p) {
    const size_t nB = (size_t)p.Kw * p.L;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nB) {
        float v = p.first ? 0.f : p.accB[e];
        for (int g = 0; g < p.ngran; ++g) v += p.partB[(size_t)g * nB + e];
        if (!p.last) {
            p.accB[e] = v;
            return;
        }
        const int row = (int)(e / p.L), f = (int)(e - (size_t)row * p.L);
        if (row < p.J) {
            if (p.dWv) p.dWv[(size_t)row * p.L + f] = v;
        } else if (row < 2 * p.J) {
            if (p.dWu) p.dWu[(size_t)(row - p.J) * p.L + f] = v;
        } else if (row < 2 * p.J + p.C) {
            if (p.dwk) p.dwk[(size_t)(row - 2 * p.J) * p.L + f] = v;
        }
        return;
    }
    const size_t i = e - nB;
    if (i >= (size_t)p.NPA) return;
    float v = p.first ? 0.f : p.accA[i];
#pragma unroll 8
    for (int tl = 0; tl < p.ntiles; ++tl) v += p.partA[(size_t)tl * p.NPA + i];
    if (!p.last) {
        p.accA[i] = v;
        return;
    }
    const int k = (int)i, o_dbv = p.C * p.D, o_dbu = o_dbv + p.J, o_dba = o_dbu + p.J;
    if (k < o_dbv) {
        if (p.dwa) p.dwa[k] = v;
    } else if (k < o_dbu) {
        if (p.dbv) p.dbv[k - o_dbv] = v;
    } else if (k < o_dba) {
        if (p.dbu) p.dbu[k - o_dbu] = v;
    } else if (p.dba) {
        p.dba[k - o_dba] = v;
    }
}

}  // namespace mcgmil

namespace {

using mcgmil_detail::fail;
using mcgmil_detail::hip_fail;

uint32_t drop_threshold(float p) {      // as in mcgmil.hip (oracle/philox_oracle.c)
    const double pd = (double)p;
    if (!(pd > 0.0)) return 0u;
    const double x = floor(pd * 65536.0 + 0.5);
    return x >= 65536.0 ? 65536u : (uint32_t)x;
}

float dropout_scale(float p) {
    const double pd = (double)p;
    return pd >= 1.0 ? 0.0f : 1.0f / (float)(1.0 - pd);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Checked size arithmetic: `ok` goes false on overflow and stays false.
struct Sizer {
    bool ok = true;
    size_t mul(size_t a, size_t b) {
        size_t r = 0;
        if (__builtin_mul_overflow(a, b, &r)) ok = false;
        return ok ? r : 0;
    }
    size_t add(size_t a, size_t b) {
        size_t r = 0;
        if (__builtin_add_overflow(a, b, &r)) ok = false;
        return ok ? r : 0;
    }
    size_t block(size_t words) { return add(mul(words, 4), 255) / 256 * 256; }   // fp32 words -> 256-byte block
};

struct GradLayout {
    int BM, K2, Kw, NPA;
    long long gran_total, gran_chunk, Rc;
    size_t wt_off, rowinfo_off, dp_off, parta_off, partb_off, acca_off, accb_off, ra_off, total;
};

int validate(const mcgmil_grad_args* a, mcgmil_args& f) {
    if (!a) return fail(MCGMIL_E_INVALID, "args is NULL");
    f = a->fwd;
    f.flags = 0;            // the forward call's outputs, launch path and scratch are not used here
    f.reserved = 0;
    f.debug = nullptr;
    size_t fwd_ws = 0;
    if (int rc = mcgmil_workspace_size(&f, &fwd_ws)) return rc;     // sizes, T, bags, probabilities
    if (f.h_dtype != MCGMIL_F32) return fail(MCGMIL_E_UNSUPPORTED, "the backward pass is built for fp32 H only");
    if (f.keep_feat || f.keep_att) return fail(MCGMIL_E_UNSUPPORTED, "the backward pass draws its own masks: replay masks are not supported");
    if (a->chunk_pairs < 0) return fail(MCGMIL_E_INVALID, "chunk_pairs must be >= 0");
    if (a->reserved != 0) return fail(MCGMIL_E_INVALID, "reserved must be 0");
    return MCGMIL_OK;
}

int layout_for(const mcgmil_grad_args* a, const mcgmil_args& f, GradLayout& l) {
    Sizer z;
    const size_t J = z.mul((size_t)f.G, (size_t)f.D);
    if (!z.ok || J > (1u << 20)) return fail(MCGMIL_E_UNSUPPORTED, "G * D too large");
    l.K2 = (int)(2 * J);
    l.Kw = l.K2 + 16;
    l.NPA = f.C * f.D + l.K2 + f.C;
    l.BM = mcgmil::grad_rows_lds_bytes(32, f.L, l.K2, l.NPA) <= 160 * 1024   ? 32
           : mcgmil::grad_rows_lds_bytes(16, f.L, l.K2, l.NPA) <= 160 * 1024 ? 16
                                                                              : 0;
    if (!l.BM) return fail(MCGMIL_E_UNSUPPORTED, "L and G * D too large for the backward row tile (160 KiB of LDS)");
    const long long cap = a->chunk_pairs ? a->chunk_pairs : MCGMIL_GRAD_DEFAULT_CHUNK_PAIRS;
    l.gran_total = (f.total_rows + MCGMIL_GRAD_GRANULE_ROWS - 1) / MCGMIL_GRAD_GRANULE_ROWS;
    l.gran_chunk = cap / ((long long)f.T * MCGMIL_GRAD_GRANULE_ROWS);
    if (l.gran_chunk < 1) l.gran_chunk = 1;
    if (l.gran_chunk > l.gran_total) l.gran_chunk = l.gran_total;
    l.Rc = l.gran_chunk * MCGMIL_GRAD_GRANULE_ROWS;
    if (l.Rc > (1ll << 30)) return fail(MCGMIL_E_UNSUPPORTED, "more than 2^30 rows per launch chunk (lower chunk_pairs)");
    const size_t Rc = (size_t)l.Rc, Kw = (size_t)l.Kw, L = (size_t)f.L;
    size_t o = 0;
    l.wt_off = o;       o = z.add(o, z.block(z.mul(L, (size_t)l.K2)));
    l.rowinfo_off = o;  o = z.add(o, z.block(z.mul(Rc, 2)));
    l.dp_off = o;       o = z.add(o, z.block(z.mul(z.mul(Rc, (size_t)f.T), Kw)));
    l.parta_off = o;    o = z.add(o, z.block(z.mul(Rc / (size_t)l.BM, (size_t)l.NPA)));
    l.partb_off = o;    o = z.add(o, z.block(z.mul(z.mul((size_t)l.gran_chunk, Kw), L)));
    l.acca_off = o;     o = z.add(o, z.block((size_t)l.NPA));
    l.accb_off = o;     o = z.add(o, z.block(z.mul(Kw, L)));
    l.ra_off = o;       o = z.add(o, z.block(z.mul(z.mul((size_t)f.num_bags, (size_t)f.T), (size_t)f.C)));
    l.total = o;
    if (!z.ok || z.mul(z.mul(Rc, (size_t)f.T), Kw) > (size_t)1 << 40)
        return fail(MCGMIL_E_UNSUPPORTED, "backward workspace too large (lower chunk_pairs or T)");
    return MCGMIL_OK;
}

template <int RT>
int launch_rows(const mcgmil::GradParams& gp, size_t lds, hipStream_t s) {
    auto* k = &mcgmil::grad_rows_kernel<RT>;
    if (int rc = mcgmil_detail::raise_lds_limit(reinterpret_cast<const void*>(k), "grad_rows_kernel LDS limit")) return rc;
    const int tiles = (gp.rows + 16 * RT - 1) / (16 * RT);
    hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(mcgmil::kGradThreads), lds, s, gp);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCGMIL_OK : hip_fail(e, "grad_rows_kernel launch");
}

}  // namespace

extern "C" {

size_t mcgmil_grad_args_size(void) { return sizeof(mcgmil_grad_args); }

int mcgmil_grad_workspace_size(const mcgmil_grad_args* a, size_t* bytes) {
    mcgmil_args f;
    if (int rc = validate(a, f)) return rc;
    if (!bytes) return fail(MCGMIL_E_INVALID, "bytes is NULL");
    GradLayout l;
    if (int rc = layout_for(a, f, l)) return rc;
    *bytes = l.total;
    return MCGMIL_OK;
}

int mcgmil_head_backward(const mcgmil_grad_args* a, void* stream) {
    mcgmil_args f;
    if (int rc = validate(a, f)) return rc;
    GradLayout l;
    if (int rc = layout_for(a, f, l)) return rc;
    if (!f.H && f.total_rows > 0) return fail(MCGMIL_E_INVALID, "H is NULL");
    if (!f.Wv || !f.Wu || !f.bv || !f.bu || !f.wa || !f.ba || !f.wk)
        return fail(MCGMIL_E_INVALID, "NULL parameter pointer");
    if (!a->A || !a->Y || !a->dY) return fail(MCGMIL_E_INVALID, "A, Y and dY are required");
    if (f.ldh < f.L) return fail(MCGMIL_E_INVALID, "ldh must be >= L");
    if (a->dH && a->ldh_grad < f.L) return fail(MCGMIL_E_INVALID, "ldh_grad must be >= L");
    if (!aligned16(f.H) || (f.ldh * 4) % 16 != 0) return fail(MCGMIL_E_ALIGN, "H and its row stride must be 16-byte aligned");
    if (!aligned16(f.Wv) || !aligned16(f.Wu) || !aligned16(f.wk) || !aligned16(f.bv) || !aligned16(f.bu) || !aligned16(f.wa))
        return fail(MCGMIL_E_ALIGN, "Wv, Wu, wk, bv, bu and wa must be 16-byte aligned");
    if (a->dH && (!aligned16(a->dH) || (a->ldh_grad * 4) % 16 != 0))
        return fail(MCGMIL_E_ALIGN, "dH and its row stride must be 16-byte aligned");
    if (!a->workspace || a->workspace_bytes < l.total)
        return fail(MCGMIL_E_WORKSPACE, "workspace missing or smaller than mcgmil_grad_workspace_size()");
    if (((uintptr_t)a->workspace & 255u) != 0) return fail(MCGMIL_E_ALIGN, "workspace must be 256-byte aligned");

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(a->workspace);
    mcgmil::GradParams gp;
    gp.H = static_cast<const float*>(f.H);
    gp.ldh = f.ldh;
    gp.bag_off = f.bag_offsets;
    gp.bag_ids = f.bag_ids;
    gp.bag_base = f.bag_id_base;
    gp.t_base = f.t_base;
    gp.B = f.num_bags; gp.T = f.T; gp.L = f.L; gp.D = f.D; gp.C = f.C; gp.G = f.G;
    gp.J = f.G * f.D; gp.K2 = l.K2; gp.Kw = l.Kw;
    gp.Wv = f.Wv; gp.Wu = f.Wu; gp.bv = f.bv; gp.bu = f.bu; gp.wa = f.wa; gp.wk = f.wk;
    gp.WT = reinterpret_cast<const float*>(ws + l.wt_off);
    gp.A = a->A; gp.Y = a->Y; gp.dY = a->dY; gp.dA = a->dA;
    gp.rA = a->dA ? reinterpret_cast<const float*>(ws + l.ra_off) : nullptr;
    gp.sf = dropout_scale(f.p_feat);
    gp.sa = dropout_scale(f.p_att);
    gp.thr_f = drop_threshold(f.p_feat);
    gp.thr_a = drop_threshold(f.p_att);
    gp.k0 = (uint32_t)f.seed;
    gp.k1 = (uint32_t)(f.seed >> 32);
    gp.Rc = (int)l.Rc;
    gp.rowinfo = reinterpret_cast<int2*>(ws + l.rowinfo_off);
    gp.dP = reinterpret_cast<float*>(ws + l.dp_off);
    gp.partA = reinterpret_cast<float*>(ws + l.parta_off);
    gp.NPA = l.NPA;
    gp.partB = reinterpret_cast<float*>(ws + l.partb_off);
    gp.dH = a->dH;
    gp.lddh = a->ldh_grad;

    mcgmil::ReduceParams rp;
    rp.partA = gp.partA; rp.partB = gp.partB;
    rp.accA = reinterpret_cast<float*>(ws + l.acca_off);
    rp.accB = reinterpret_cast<float*>(ws + l.accb_off);
    rp.NPA = l.NPA; rp.Kw = l.Kw; rp.L = f.L; rp.J = gp.J; rp.C = f.C; rp.D = f.D;
    rp.dWv = a->dWv; rp.dbv = a->dbv; rp.dWu = a->dWu; rp.dbu = a->dbu;
    rp.dwa = a->dwa; rp.dba = a->dba; rp.dwk = a->dwk;
    const unsigned rblocks = (unsigned)(((size_t)l.Kw * f.L + l.NPA + 255) / 256);
    hipError_t e;

    if (f.total_rows > 0) {
        if (a->dH) {
            const size_t total = (size_t)f.L * l.K2;
            hipLaunchKernelGGL(mcgmil::grad_pack_kernel, dim3((unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048)),
                               dim3(256), 0, s, f.Wv, f.Wu, f.L, gp.J, reinterpret_cast<float*>(ws + l.wt_off));
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "grad_pack_kernel launch");
        }
        if (a->dA) {
            hipLaunchKernelGGL(mcgmil::grad_ra_kernel, dim3((unsigned)f.num_bags, (unsigned)(f.T * f.C)), dim3(256), 0, s,
                               f.bag_offsets, f.T, f.C, a->A, a->dA, reinterpret_cast<float*>(ws + l.ra_off));
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "grad_ra_kernel launch");
        }
    }
    const size_t lds = mcgmil::grad_rows_lds_bytes(l.BM, f.L, l.K2, l.NPA);
    long long g0 = 0;
    do {
        const long long ng = l.gran_total - g0 < l.gran_chunk ? l.gran_total - g0 : l.gran_chunk;
        gp.row0 = g0 * MCGMIL_GRAD_GRANULE_ROWS;
        const long long left = f.total_rows - gp.row0;
        gp.rows = (int)(left < ng * MCGMIL_GRAD_GRANULE_ROWS ? left : ng * MCGMIL_GRAD_GRANULE_ROWS);
        if (gp.rows > 0) {
            if (int rc = l.BM == 32 ? launch_rows<2>(gp, lds, s) : launch_rows<1>(gp, lds, s)) return rc;
            hipLaunchKernelGGL(mcgmil::grad_weights_kernel, dim3((unsigned)((f.L + 63) / 64), (unsigned)((l.Kw + 63) / 64), (unsigned)ng),
                               dim3(mcgmil::kWThreads), 0, s, gp);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "grad_weights_kernel launch");
        }
        rp.ntiles = (gp.rows + l.BM - 1) / l.BM;
        rp.ngran = (int)ng;
        rp.first = g0 == 0;
        rp.last = g0 + ng >= l.gran_total;
        hipLaunchKernelGGL(mcgmil::grad_reduce_kernel, dim3(rblocks), dim3(256), 0, s, rp);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "grad_reduce_kernel launch");
        g0 += ng;
    } while (g0 < l.gran_total);
    return MCGMIL_OK;
}

}  // extern "C"
