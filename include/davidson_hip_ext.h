/* davidson_hip_ext.h - extension entries of libdavidson_hip.so, next to the C ABI of davidson_hip.h (DAV_HIP_ABI_VERSION 109, which
 * this header neither changes nor extends: its table of dav_* entries stays as it is, entry for entry).  Extension entries carry the
 * prefix davx_; they follow every convention of davidson_hip.h (return 0 or non-zero with dav_last_error(), host pointers unless the
 * name says _dev, the engine behind dav_handle_t) and are exported by both builds of the library.  Their mirrors: the table EXT of
 * fortran_davidson_amd/_abi.py, the interface bodies name="davx_*" of fortran/davidson_hip_c.f90 and the doors name="fdx_*" of
 * fortran/davidson_c_api.f90 (tests/test_coo_cpu.py compares them with this header). */
#ifndef DAVIDSON_HIP_EXT_H
#define DAVIDSON_HIP_EXT_H

#include "davidson_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same matrix as COO TRIPLES (row_idx[p], col_idx[p], vals[p]), p = 0 .. nnz - 1, in ANY order, duplicates included: what an assembly
 * loop emits, an uncoalesced torch.sparse_coo_tensor, a scipy coo_matrix.  Additive to ABI 109: no entry, constant or
 * field of dav_stats of davidson_hip.h changes.  DEFINITION: the ROW FORM of the triples is the CSR matrix obtained by a STABLE sort of the triples by row;
 * both entries build, bit for bit, what dav_set_operator_csr builds from the row form with the same index_base and triangle - row offsets,
 * columns, values, the diagonal (duplicates summed in ascending p from +0.0), the work list, with DAV_CSR_DIAGONALS the decision, the
 * refusal and the storage by diagonals.  Duplicates are never coalesced: they stay separate terms in the order of p.  Symmetry of
 * DAV_CSR_FULL input stays the caller's promise.  Every rank passes the GLOBAL triples; which = DAV_OP_A, DAV_OP_B or DAV_OP_M; index_base
 * applies to both index arrays; nnz == 0 is valid with null arrays.  The kind of the operator is DAV_KIND_CSR (DAV_KIND_DIA with the flag).
 * REFUSALS, each before anything is allocated for the operator, each leaving the operator UNSET and the engine usable (dav_last_error):
 * nnz < 0; nnz >= 2^32 (the position p is the 32-bit tie of the sort key); a null array with nnz > 0; a bad index_base, triangle, row_bits
 * or col_bits; a row index out of range; a column index out of range; an entry above the diagonal with DAV_CSR_LOWER.  For the rules on
 * entries the FIRST offending triple (the smallest p) is named, with the caller's row and column in the caller's base, and both entries
 * give the same text.  VALUE MAP: after dav_keep_value_map(h, which, 1) the map and the diagonal sources name the positions of the
 * TRIPLES, so dav_update_operator_values(_dev) takes vals in the order of the triples and equals, bit for bit, a fresh COO set call.
 * davx_set_operator_coo (host arrays) validates, sorts the triples by row with a stable counting sort on the host and continues as
 * dav_set_operator_csr does.
 * davx_set_operator_coo_dev (device arrays of the engine's device; row_idx and col_idx each of 32- or 64-bit signed integers) builds the
 * operator on the GPU: the pointers are checked before any launch, lengths included (the message names row_idx, col_idx or vals); one
 * entry pass finds the first offending triple and counts the entries per row, a scan gives the offsets, every entry takes an atomic
 * slot of its row with the key  column << 32 | p,  and each row is sorted by key - the keys are unique, so the slot order leaves no
 * trace; rows of at most 64 entries are sorted by one wave in registers, longer ones by the sorts of dav_set_operator_csr_dev.  The
 * diagonal entries form a second small pattern sorted by p and summed per row.  No floating-point atomics; no result depends on the order
 * in which atomics land; the same bits on any rank count.  The triples must be COMPLETE when the call is made; the call returns after
 * the engine has stopped reading them.  Scratch comes from the engine's allocator and is released before return: 16 bytes per row of
 * this rank and 32 per row of the matrix, 4 bytes per entry of this rank, 16 per diagonal entry, with DAV_CSR_DIAGONALS 2 n - 1 bytes
 * of marks, and 32 bytes per entry of the longest row above 2048 entries. */
int davx_set_operator_coo(dav_handle_t h, int which, int64_t nnz, const int32_t* row_idx, const int32_t* col_idx, const double* vals,
                         int index_base /* 0 or 1 */, int triangle /* as dav_set_operator_csr */);
int davx_set_operator_coo_dev(dav_handle_t h, int which, int64_t nnz, const void* row_idx, int row_bits /* 32 | 64 */, const void* col_idx,
                             int col_bits /* 32 | 64 */, const double* vals, int index_base /* 0 or 1 */, int triangle);

#ifdef __cplusplus
}
#endif
#endif
