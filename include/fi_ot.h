/*
 * fi_ot.h -- C ABI of libfi_ot.so: the Sinkhorn term of the intertwiner loss differentiated through its iterations
 * (OptTrans(no_bp_P_L=False)), MI355X (gfx950).  A library of its own next to libfi_hip.so (include/fi_capi.h), which
 * it links against and whose conventions it follows: device pointers, a hipStream_t as void*, caller-allocated
 * outputs and workspaces, no host synchronisation, FI_OK or a negative FI_ERR_* status with the message in
 * libfi_hip's fi_last_error().  The detached form (the reference default) stays fi_sinkhorn_forward of fi_capi.h.
 */
#ifndef FI_OT_H_
#define FI_OT_H_

#include "fi_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Bytes of workspace fi_ot_sinkhorn_backprop needs.  HOST function, no GPU work.
 * Replaces: the autograd tape of the L iterations of _sinkhorn_iterate  lib/OT_module.py:104-135 (:121-127, the loop).
 * Per problem (4 L + 1) vectors of 256 floats: a_1..a_L, b_0..b_L and the two adjoint vectors of every iteration
 * (201 KiB at L = 50), and the 256 x 256 cost matrix (256 KiB).  0 for arguments the launch entry refuses (S outside [1, 256], L < 1, num_problems < 0).
 * ---------------------------------------------------------------------- */
size_t fi_ot_sinkhorn_backprop_workspace_bytes(int num_problems, int S, int L);

/* ------------------------------------------------------------------------
 * loss and d loss / d C of num_problems Sinkhorn problems, the plan NOT detached.
 * Replaces: _sinkhorn_iterate  lib/OT_module.py:104-135 with no_bp_P_L=False (:129-131 skipped) and torch's backward
 *           through its 2 L mat-vecs, up to the cost matrix.
 * x, y [num_problems, S, D], eps_inv, L, cost_mode (0 cosine with the normaliser inside, 1 l2, 2 dot on rows the
 * caller normalised): as fi_sinkhorn_forward.  1 <= S <= 256, D >= 1, L >= 1.
 * Outputs: loss [num_problems], bit-equal to fi_sinkhorn_forward's; dcost [num_problems, S, S] = d loss / d C with
 *   loss = sum (a_L K b_L^T) o C,  K = exp(-eps_inv C),  b_0 = 1/S,  a_l = (1/S) / (K b_{l-1} + 1e-20),
 *   b_l = (1/S) / (K^T a_l + 1e-20):   dcost = P o (1 - eps_inv C) - eps_inv K o M,  M the rank-2L sum of the reverse
 * sweep (csrc/sinkhorn_bp.hip).  dcost has entries of either sign.  The chain from C to x, y is the caller's, as for
 * the plan of fi_sinkhorn_forward.
 * workspace: fi_ot_sinkhorn_backprop_workspace_bytes(num_problems, S, L) bytes, 16-byte aligned; workspace_bytes is
 * the size of the buffer passed.  Nothing beyond that many bytes, loss and dcost is written.  One launch, no atomics:
 * the bits of a problem's outputs do not depend on the other problems of the launch.
 * Status: FI_ERR_INVALID_ARG for L < 1, D < 1, a cost_mode outside {0, 1, 2}, a null pointer, a workspace that is
 * misaligned or smaller than the query's answer; FI_ERR_UNSUPPORTED for S outside [1, 256] -- the codes of
 * fi_sinkhorn_forward, returned before anything is launched.
 * ---------------------------------------------------------------------- */
int fi_ot_sinkhorn_backprop(const float *x, const float *y, int num_problems, int S, int D, float eps_inv, int L,
                            int cost_mode, float *loss, float *dcost, void *workspace, size_t workspace_bytes,
                            fi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FI_OT_H_ */
