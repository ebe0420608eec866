/* davidson_hip_bprecond.h - a BLOCK preconditioner built by the engine from stored BSR operators: extension entries of libdavidson_hip.so
 * next to the C ABI of davidson_hip.h (DAV_HIP_ABI_VERSION 109, which this header neither changes nor extends), to davidson_hip_ext.h,
 * davidson_hip_herm.h and davidson_hip_precond.h.  The entries carry the prefix davq_; they follow every convention of davidson_hip.h
 * (return 0 or non-zero with dav_last_error(), host pointers, the engine behind dav_handle_t) and are exported by both builds of the
 * library.  Their mirrors: the table BPRECOND of fortran_davidson_amd/_abi.py, the interface bodies name="davq_*" of
 * fortran/davidson_hip_c.f90 and the doors name="fdq_*" of fortran/davidson_c_api.f90 (tests/test_bfsai_cpu.py compares them with this
 * header).  davp_build_fsai of davidson_hip_precond.h serves CSR operators and is not changed by anything here. */
#ifndef DAVIDSON_HIP_BPRECOND_H
#define DAVIDSON_HIP_BPRECOND_H

#include "davidson_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE BLOCK FACTORIZED SPARSE APPROXIMATE INVERSE.  For C = A - sigma B symmetric positive definite the build gives a block
 * lower-triangular G with (G C G^T)_II = I_b for every block row I and puts M = G^T G, symmetric positive definite by construction, into
 * slot DAV_OP_M, where DAV_METHOD_DPR and DAV_METHOD_GJD apply it as they apply any operator of that slot.
 * DEFINITION.  A is the operator of slot DAV_OP_A, a BSR operator of block size b (dav_set_operator_bsr(_dev); a complex Hermitian
 * operator set by davh_set_operator_csr(_dev) is one with b = 2); B is the operator of slot DAV_OP_B - a BSR operator of the same b, or
 * the identity when the slot is unset or holds the identity; sigma is finite; level is 1, 2 or 3; one rank; nb = n / b.
 *   PATTERN, at block level.  P_1(I) = the distinct block columns J <= I of block row I of the canonical store of A, and I itself if the
 *   block row does not store it.  P_L(I) = the union of P_1(J) over J in P_{L-1}(I), ascending, I last: the rule of davp_build_fsai
 *   applied to the block index arrays.  B does not contribute.  With m = |P_level(I)| and s = m b: a block row with s > 64 is refused -
 *   the smallest such block row, its m and b are named - never cut.
 *   BLOCK ROW.  J = P_level(I).  The scalar index p = q b + r stands for row r of block J_q.  For p' <= p, C[p][p'] =
 *   A(J_q b + r, J_q' b + r') - sigma * B(same), where A(., .) is the sum, from +0.0 in stored order, of the stored blocks of block row J_q
 *   with block column J_q' (duplicate blocks are separate terms); of a diagonal block only the lower triangle is read.  C = L L^T by a
 *   Cholesky factorisation in a fixed operation order (column by column, right-looking).  A pivot that is not finite or not > 0 refuses
 *   the call: "A - sigma B is not positive definite on the pattern of block row I", I the smallest such block row, numbered from 0.  Then
 *   L^T X = E, E the last b columns of the identity of order s: b back substitutions from the last row up, no forward solve and no second
 *   factorisation.  G(I b + t, J_q b + r) = X[q b + r][t]: the block row of G is the last b rows of L^-1.  Its diagonal block is lower
 *   triangular; the entries above its diagonal are stored as +0.0.  For b = 1 this is the G of davp_build_fsai up to rounding (the
 *   operation order differs).  With every stored block dense it is, mathematically, the G that davp_build_fsai builds from the same
 *   matrix expanded to CSR: the lower triangle of a block pattern is that scalar pattern, and the inverse Cholesky factor of a leading
 *   principal submatrix is the leading submatrix of the inverse factor.
 *   RESULT.  Slot DAV_OP_M holds an operator of an internal kind (DAV_KIND_BFSAI) made of two canonical BSR stores of block size b, the
 *   block rows of G and the block rows of G^T; dav_apply(h, DAV_OP_M, ...) computes dst = G^T (G src), bit for bit what two applies give
 *   with the slot set to the two factors as BSR operators (davq_block_fsai_get_factor).  The operator is a SNAPSHOT of A, B and sigma
 *   at the call; calling the entry again replaces it; any set call on DAV_OP_M replaces it and releases both stores.  Two builds from
 *   the same operators give the same bits: no floating-point atomics are used, only integer ones over row numbers and slots.
 * REFUSALS, each through dav_last_error(), each before anything is allocated for the operator, each leaving slot DAV_OP_M UNSET and the
 * engine usable: A not set or not a BSR operator (the message names the kind); B set and neither a BSR operator of the block size of A
 * nor the identity; level outside 1..3; sigma not finite; an engine of several ranks ("a rank stores only its rows of A and a row of G
 * needs other rows"); a block row of more than 64 scalar columns; a failed pivot.  With the built operator in the slot,
 * dav_update_operator_values(_dev), dav_keep_value_map(h, DAV_OP_M, 1) and dav_get_diagonal refuse with a message that names the kind.
 * DAV_METHOD_BDPR, _CHEB and _LCHEB ignore the slot as before. */
int davq_build_block_fsai(dav_handle_t h, double sigma, int level /* 1..3 */);
/* the block size, the blocks of G, the longest block row of G and of G^T (in blocks); all zero when slot DAV_OP_M holds no built block FSAI */
int davq_block_fsai_info(dav_handle_t h, int* block_size, int64_t* nnzb, int64_t* longest_row, int64_t* longest_col);
/* G as 0-based BSR with row-major blocks into caller-allocated host arrays (n / b + 1 offsets, nnzb block columns, nnzb b b values), moved
 * and never computed with: the arrays go straight back into dav_set_operator_bsr; transposed != 0: the store of G^T */
int davq_block_fsai_get_factor(dav_handle_t h, int transposed, int64_t* block_row_ptr, int32_t* block_col_idx, double* vals);

#ifdef __cplusplus
}
#endif
#endif
