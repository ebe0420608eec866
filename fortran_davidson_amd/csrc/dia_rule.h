// Storage by diagonals of a CSR operator (DAV_CSR_DIAGONALS), the host side of the decision: the set of offsets column - row of the
// canonical matrix and the rule that admits it.  Plain C++ (no HIP): engine_sparse.hip includes it, and so can a stand-alone program.
//
// The set is taken from the GLOBAL arrays every rank is given, through a table of 2 n - 1 marks (mark[off + n - 1] = 1): the host entry
// fills the table with dia_mark_host, the device entry with launch_dia_mark (k_dia.hip) and reads it back; dia_offsets_from_marks then
// gives both the same sorted list.  With DAV_CSR_LOWER an entry below the diagonal marks its mirror image too.
//
// The rule, a design constant: the matrix is stored by diagonals when  nd * n <= DIA_MAX_FILL * max(entries, n)  with entries = the
// entries of the canonical matrix (duplicates counted, mirrored images included).  A slot costs 8 bytes, a CSR entry 12: DIA_MAX_FILL = 4
// admits at most 32 stored bytes per entry; beyond that the format reads more than it saves.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

constexpr int DIA_MAX_FILL = 4;

inline bool dia_eligible(int64_t nd, int64_t n, int64_t entries) {
  return nd * n <= (int64_t)DIA_MAX_FILL * std::max(entries, n);          // nd < 2^32, n < 2^31: no overflow
}

inline std::string dia_refusal(int64_t nd, int64_t n, int64_t entries) {
  return "DAV_CSR_DIAGONALS: the matrix has nd = " + std::to_string(nd) + " diagonals and " + std::to_string(entries) +
         " entries; it is stored by diagonals only when nd * n <= DIA_MAX_FILL * max(entries, n) (DIA_MAX_FILL = " +
         std::to_string(DIA_MAX_FILL) + ", n = " + std::to_string(n) + ")";
}

// marks of a validated pattern (every column in range, nothing above the diagonal of a lower triangle); *ndiag = its diagonal entries
template <class RP, class CI>
void dia_mark_host(const RP* row_ptr, const CI* col_idx, int64_t n, int base, bool lower, std::vector<uint8_t>& marks, int64_t* ndiag) {
  marks.assign(n > 0 ? (size_t)(2 * n - 1) : 0, 0);
  int64_t nd = 0;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t p = (int64_t)row_ptr[i] - base; p < (int64_t)row_ptr[i + 1] - base; ++p) {
      const int64_t j = (int64_t)col_idx[p] - base;
      marks[(size_t)(j - i + n - 1)] = 1;
      if (lower) marks[(size_t)(i - j + n - 1)] = 1;
      if (j == i) ++nd;
    }
  *ndiag = nd;
}

inline void dia_offsets_from_marks(const uint8_t* marks, int64_t n, std::vector<int32_t>& offs) {
  offs.clear();
  for (int64_t t = 0; t < 2 * n - 1; ++t)
    if (marks[t]) offs.push_back((int32_t)(t - (n - 1)));
}

// entries of the canonical matrix from those of the caller's arrays
inline int64_t dia_canonical_entries(int64_t nnz, int64_t ndiag, bool lower) { return lower ? 2 * nnz - ndiag : nnz; }
