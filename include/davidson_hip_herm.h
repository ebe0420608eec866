/* davidson_hip_herm.h - complex Hermitian CSR operators through their real form: extension entries of libdavidson_hip.so next to the C ABI
 * of davidson_hip.h (DAV_HIP_ABI_VERSION 109, which this header neither changes nor extends) and to davidson_hip_ext.h.  The entries
 * carry the prefix davh_; they follow every convention of davidson_hip.h (return 0 or non-zero with dav_last_error(), host pointers unless
 * the name says _dev, the engine behind dav_handle_t) and are exported by both builds of the library.  Their mirrors: the table HERM of
 * fortran_davidson_amd/_abi.py, the interface bodies name="davh_*" of fortran/davidson_hip_c.f90 and the doors name="fdh_*" of
 * fortran/davidson_c_api.f90 (tests/test_herm_cpu.py compares them with this header). */
#ifndef DAVIDSON_HIP_HERM_H
#define DAVIDSON_HIP_HERM_H

#include "davidson_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE REAL FORM.  A Hermitian matrix H of order n_c has a real symmetric form of order n = 2 n_c: with real and imaginary parts
 * interleaved, v[2 i] = Re x_i, v[2 i + 1] = Im x_i, every entry h_ij = a + i b is the 2 x 2 block [[a, -b], [b, a]] at block (i, j) - a
 * BSR matrix with block size 2 on the pattern of the complex CSR matrix.  The block of h_ji = conj(h_ij) is the transpose of the block of
 * h_ij.  Every eigenvalue of H is an eigenvalue of the real form twice: a solve for L complex pairs is a solve for 2 L real pairs
 * (DESIGN section 28 says how the complex pairs are taken from them).
 * The engine was created with the REAL order n = 2 n_c.  row_ptr (n_c + 1 offsets) and col_idx are the pattern of H, numbered from
 * index_base; vals holds 2 nnz doubles, the pair (re, im) of entry p at vals[2 p], vals[2 p + 1] - the memory of complex128 /
 * double _Complex / complex(c_double_complex) arrays, read where it lies, 16-byte aligned.
 * DEFINITION.  Both entries build, bit for bit, the store that dav_set_operator_bsr(h, which, 2, row_ptr, col_idx, blocks, index_base,
 * triangle, DAV_BSR_ROW_MAJOR) and its _dev twin build from the same pattern and blocks[p] = [[a_p, -b_p], [b_p, a_p]]: block row offsets,
 * block columns, values, the diagonal (diag[2 i] = diag[2 i + 1] = the real parts of the diagonal entries of row i summed in input order
 * from +0.0), the work list and - after dav_keep_value_map(h, which, 1) - the value map.  The kind of the operator is DAV_KIND_BSR, and
 * everything downstream of the build serves it as it serves any BSR operator with b = 2.  -b is a sign flip: values are moved, never
 * computed with.  which = DAV_OP_A, DAV_OP_B or DAV_OP_M.  Duplicates stay separate terms in input order.  triangle = DAV_CSR_LOWER:
 * only the entries with column <= row are given and the strict lower ones are mirrored as their conjugates; DAV_CSR_FULL:
 * h_ji = conj(h_ij) is the caller's promise.  Every rank passes the global arrays.
 * REFUSALS, each before anything is kept, each leaving the operator UNSET and the engine usable, with the same text from both entries:
 * an odd engine order; a bad index_base, triangle, row_ptr_bits or col_bits; DAV_CSR_DIAGONALS (a Hermitian operator is stored by
 * blocks); null arrays; row_ptr[0] != index_base; row_ptr decreasing; a column out of range or (DAV_CSR_LOWER) above the diagonal; a
 * DIAGONAL ENTRY WHOSE IMAGINARY PART IS NOT +-0.0 (NaN included) - the first such entry (smallest p) is named with its row in the
 * caller's base and the value: the real form would not be symmetric.
 * VALUE MAP.  An operator set through these entries after dav_keep_value_map(h, which, 1) takes new values through
 * dav_update_operator_values(_dev) as 2 nnz doubles, (re, im) pairs in the order of the set call, and then equals a fresh davh_ set call
 * bit for bit; an imaginary diagonal is refused there too, before a value moves.
 * davh_set_operator_csr_dev (device arrays of the engine's device; indices of 32 or 64 bits) builds the operator on the GPU.  It holds no
 * scratch for expanded values: the caller's 16 bytes per entry are read by the diagonal pass and once by the gather. */
int davh_set_operator_csr(dav_handle_t h, int which, const int64_t* row_ptr, const int32_t* col_idx, const double* vals,
                          int index_base /* 0 or 1 */, int triangle /* DAV_CSR_FULL | DAV_CSR_LOWER */);
int davh_set_operator_csr_dev(dav_handle_t h, int which, const void* row_ptr, int row_ptr_bits /* 32 | 64 */, const void* col_idx,
                              int col_bits /* 32 | 64 */, const double* vals, int index_base /* 0 or 1 */, int triangle);

#ifdef __cplusplus
}
#endif
#endif
