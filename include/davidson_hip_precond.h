/* davidson_hip_precond.h - a preconditioner BUILT by the engine from the stored operators: extension entries of libdavidson_hip.so next to
 * the C ABI of davidson_hip.h (DAV_HIP_ABI_VERSION 109, which this header neither changes nor extends), to davidson_hip_ext.h and to
 * davidson_hip_herm.h.  The entries carry the prefix davp_; they follow every convention of davidson_hip.h (return 0 or non-zero with
 * dav_last_error(), host pointers, the engine behind dav_handle_t) and are exported by both builds of the library.  Their mirrors: the
 * table PRECOND of fortran_davidson_amd/_abi.py, the interface bodies name="davp_*" of fortran/davidson_hip_c.f90 and the doors
 * name="fdp_*" of fortran/davidson_c_api.f90 (tests/test_fsai_cpu.py compares them with this header). */
#ifndef DAVIDSON_HIP_PRECOND_H
#define DAVIDSON_HIP_PRECOND_H

#include "davidson_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE FACTORIZED SPARSE APPROXIMATE INVERSE (FSAI; Kolotilina and Yeremin).  For C = A - sigma B symmetric positive definite the build
 * gives a sparse lower-triangular G with diag(G C G^T) = 1 and puts M = G^T G, symmetric positive definite by construction, into slot
 * DAV_OP_M - where DAV_METHOD_DPR and DAV_METHOD_GJD apply it as they apply any operator of that slot (davidson_hip.h).
 * DEFINITION.  A is the operator of slot DAV_OP_A, a CSR operator (set by dav_set_operator_csr(_dev) or davx_set_operator_coo(_dev)
 * without DAV_CSR_DIAGONALS); B is the operator of slot DAV_OP_B - a CSR operator, or the identity when the slot is unset or holds the
 * identity; sigma is finite; level is 1, 2 or 3.
 *   PATTERN.  P_1(i) = the distinct columns j <= i of row i of the canonical store of A, and i itself if the row does not store it.
 *   P_L(i) = the union of P_1(j) over j in P_{L-1}(i) (all of them <= i): the pattern of tril(A)^L, the L-th power of the LOWER TRIANGLE
 *   of A, ascending, i last - column j is in it when a path i = k_0 >= k_1 >= ... >= k_L = j runs over stored entries (or stays in
 *   place).  It is narrower than tril(A^L), whose paths may pass through rows above i: on the 5-point Laplacian a row holds at most 3,
 *   6 and 10 columns at levels 1, 2 and 3 where tril(A^L) holds 3, 7 and 13.  B does not contribute.  A row whose pattern holds more
 *   than 64 columns is refused - the smallest such row and its length are named - never cut.
 *   ROW.  J = P_level(i), m = |J|.  C_JJ[p][q] = A(J_p, J_q) - sigma * B(J_p, J_q) for q <= p, where A(r, c) is the sum, from +0.0 in
 *   stored order, of every stored entry of row r with column c (duplicates are separate terms, as everywhere in the engine).  C_JJ = L L^T
 *   by a Cholesky factorisation in a fixed operation order (column by column, right-looking); C_JJ y = e_m by z = e_m / l_mm and the back
 *   substitution of L^T y = z from the last row up; G(i, J) = y / sqrt(y_m).  A pivot that is not finite or not > 0 refuses the call:
 *   "A - sigma B is not positive definite on the pattern of row i", i the smallest such row, numbered from 0.
 *   RESULT.  Slot DAV_OP_M holds an operator of an internal kind made of two canonical CSR stores, the rows of G and the rows of G^T;
 *   dav_apply(h, DAV_OP_M, ...) computes dst = G^T (G src), bit for bit what two applies give with the slot set to the two factors as CSR
 *   operators (davp_fsai_get_factor).  The operator is a SNAPSHOT of A, B and sigma at the call: later dav_update_operator_values on A or
 *   B do not change it; calling davp_build_fsai again replaces it; any set call on DAV_OP_M replaces it and releases both stores.  Two
 *   builds from the same operators give the same bits.
 * REFUSALS, each through dav_last_error(), each before anything is allocated for the operator, each leaving slot DAV_OP_M UNSET and the
 * engine usable: A not set or not a CSR operator (BSR - a Hermitian operator too -, a CSR matrix stored by diagonals, dense, generated and
 * callback operators; the message names the kind); B set and neither CSR nor the identity; level outside 1..3; sigma not finite; an
 * engine of several ranks ("a rank stores only its rows of A and a row of G needs other rows"); a pattern row of more than 64 columns; a
 * failed pivot.  With the built operator in the slot, dav_update_operator_values(_dev), dav_keep_value_map(h, DAV_OP_M, 1) and
 * dav_get_diagonal refuse with a message that names the kind.  DAV_METHOD_BDPR, _CHEB and _LCHEB ignore the slot as before. */
int davp_build_fsai(dav_handle_t h, double sigma, int level /* 1..3 */);
/* nnz of G, the longest row of G, the longest row of G^T; all zero when slot DAV_OP_M does not hold a built FSAI */
int davp_fsai_info(dav_handle_t h, int64_t* nnz, int64_t* longest_row, int64_t* longest_col);
/* G as 0-based CSR into caller-allocated host arrays (n + 1 offsets, nnz columns, nnz values); transposed != 0: the store of G^T */
int davp_fsai_get_factor(dav_handle_t h, int transposed, int64_t* row_ptr, int32_t* col_idx, double* vals);

#ifdef __cplusplus
}
#endif
#endif
