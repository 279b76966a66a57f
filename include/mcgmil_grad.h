/*
 * mcgmil_grad.h -- C ABI of the backward pass of the MI355X (gfx950) MCDO gated-attention MIL
 * head: the gradients of mcgmil_mcdo_forward (include/mcgmil.h) with respect to the features H
 * and the seven head parameters, for all T dropout samples of every bag in one call.
 *
 * Reference interfaces served (the reference trains through torch autograd; there is no FFI):
 *   mcgmil_head_backward  <- loss.backward() through MultiHeadGatedAttentionMIL.forward in train
 *                            mode (model.py:211-253) from H on, as net_utils.train_gacc, main.py
 *                            and cross_validation.py run it
 *
 * Nothing but H, A, Y and the seed has to be kept from the forward call: every dropout mask is a
 * pure function of (seed, bag counter, sample counter, row, column) and is drawn again here from
 * the same Philox stream. Operands are fp32 (the reference's precision); the result is
 * deterministic (no floating-point atomics: two calls with the same arguments are bitwise equal,
 * whatever chunk_pairs is).
 *
 * Conventions are those of mcgmil.h: device pointers, caller-owned buffers, stream-ordered
 * launches without host synchronisation, 0 or a negative MCGMIL_E* code with the message in
 * mcgmil_last_error(). This header adds entry points only; mcgmil_args and MCGMIL_ABI_VERSION
 * are unchanged.
 */
#ifndef MCGMIL_GRAD_H_
#define MCGMIL_GRAD_H_

#include "mcgmil.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of H per split-K granule of the weight-gradient GEMM: a launch chunk is a whole number
 * of granules, and every partial sum is tied to a granule (or to a row tile inside one), so the
 * summation order does not depend on how the launcher chunks the call. */
#define MCGMIL_GRAD_GRANULE_ROWS 512
/* Default cap on the (sample, row) pairs whose gate gradients are in the workspace at once. */
#define MCGMIL_GRAD_DEFAULT_CHUNK_PAIRS 32768

typedef struct mcgmil_grad_args {
    /* The forward call these gradients belong to: sizes, H, bag_offsets, the parameters, the
     * dropout rates, seed, bag_id_base / bag_ids and t_base as passed to mcgmil_mcdo_forward.
     * h_dtype must be MCGMIL_F32 and keep_feat / keep_att NULL (MCGMIL_E_UNSUPPORTED otherwise).
     * Its output pointers, packed_w, workspace, debug and flags are ignored. */
    mcgmil_args fwd;
    /* ---- saved from the forward call ---- */
    const float* A;       /* [sum_b T*C*N_b] attention (order bag,t,c,n) */
    const float* Y;       /* [B, T, C] class logits */
    /* ---- incoming gradients ---- */
    const float* dY;      /* [B, T, C] */
    const float* dA;      /* in A's layout, or NULL (no gradient flows into A) */
    /* ---- outputs: fp32, parameter layout, OVERWRITTEN (not accumulated); each optional ---- */
    float* dWv;           /* [G, D, L] */
    float* dbv;           /* [G, D] */
    float* dWu;           /* [G, D, L] */
    float* dbu;           /* [G, D] */
    float* dwa;           /* [C, D] */
    float* dba;           /* [C] */
    float* dwk;           /* [C, L] */
    float* dH;            /* [total_rows, ldh_grad] gradient of H summed over the T samples, or NULL */
    int64_t ldh_grad;     /* row stride of dH in elements (>= L, multiple of 4) */
    /* ---- scratch ---- */
    void* workspace;      /* >= mcgmil_grad_workspace_size() bytes, 256-byte aligned */
    size_t workspace_bytes;
    /* Cap on the (sample, row) pairs per launch chunk, 0 = MCGMIL_GRAD_DEFAULT_CHUNK_PAIRS. A
     * chunk is max(1, cap / (T * MCGMIL_GRAD_GRANULE_ROWS)) granules of rows with all their T
     * samples; the launcher walks the chunks on the same stream. */
    int64_t chunk_pairs;
    int64_t reserved;     /* must be 0 */
} mcgmil_grad_args;

size_t mcgmil_grad_args_size(void);     /* sizeof(mcgmil_grad_args), for binding checks */

/* Bytes of scratch mcgmil_head_backward needs for these sizes, outputs and chunk_pairs. With
 * R_c = rows per chunk, K = 2*G*D + 16 and row tiles of 32 rows (16 when 32 do not fit the LDS):
 *   transposed gate weights L*2GD | rowinfo R_c*2 | dP R_c*T*K | row-tile partials
 *   (R_c/tile)*(C*D + 2*G*D + C) | granule partials (R_c/512)*K*L | accumulators K*L + ... |
 *   B*T*C (the sum_m A dA pre-reduction), fp32 words each, every block rounded up to 256 bytes. */
int mcgmil_grad_workspace_size(const mcgmil_grad_args* a, size_t* bytes);

/* dH and the parameter gradients of the forward call described by a->fwd. */
int mcgmil_head_backward(const mcgmil_grad_args* a, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MCGMIL_GRAD_H_ */
