// Host side of COO input (davx_set_operator_coo; the scalar checks also serve davx_set_operator_coo_dev): plain C++ without a GPU call, so
// that it also compiles into a stand-alone program under a sanitizer (tests/host_sanitizer/coo_driver.cpp).
//   coo_bad_arguments   the scalar arguments and null arrays, before anything is read ("" = fine)
//   coo_first_bad       the first triple (smallest p) with a row or column out of range or, lower, above the diagonal; -1 = none
//   coo_row_form        the ROW FORM of validated triples: a stable counting sort by row - row_ptr (numbered from base), the caller's
//                       columns and values in that order, and perm[q] = the position p of the triple that landed at q
#pragma once
#include <cstdint>
#include <string>
#include <vector>

// bits = {row_bits, col_bits} of the device entry, nullptr for the host entry
inline std::string coo_bad_arguments(int64_t n, int64_t nnz, int index_base, int triangle, int triangle_bits, const int* bits,
                                     const void* row_idx, const void* col_idx, const void* vals) {
  if (n >= ((int64_t)1 << 31)) return "n = " + std::to_string(n) + " must be below 2^31 (int32 column indices)";
  if (nnz < 0) return "nnz = " + std::to_string(nnz) + " must not be negative";
  if (nnz >= ((int64_t)1 << 32))
    return "nnz = " + std::to_string(nnz) + " must be below 2^32 (the position of a triple is the 32-bit tie of its sort key)";
  if (index_base != 0 && index_base != 1) return "index_base must be 0 or 1";
  if ((triangle & ~triangle_bits) != 0) return "triangle must be DAV_CSR_FULL or DAV_CSR_LOWER";
  if (bits && bits[0] != 32 && bits[0] != 64) return "row_bits must be 32 or 64";
  if (bits && bits[1] != 32 && bits[1] != 64) return "col_bits must be 32 or 64";
  if (nnz > 0 && !row_idx) return "null row_idx";
  if (nnz > 0 && !col_idx) return "null col_idx";
  if (nnz > 0 && !vals) return "null vals";
  return "";
}

inline int64_t coo_first_bad(int64_t n, int64_t nnz, const int32_t* row_idx, const int32_t* col_idx, int base, bool lower) {
  for (int64_t p = 0; p < nnz; ++p) {
    const int64_t i = (int64_t)row_idx[p] - base, j = (int64_t)col_idx[p] - base;
    if (i < 0 || i >= n || j < 0 || j >= n || (lower && j > i)) return p;
  }
  return -1;
}

struct CooRowForm {
  std::vector<int64_t> row_ptr, perm;
  std::vector<int32_t> col;
  std::vector<double> val;
};

inline void coo_row_form(int64_t n, int64_t nnz, const int32_t* row_idx, const int32_t* col_idx, const double* vals, int base, CooRowForm& f) {
  f.row_ptr.assign((size_t)n + 1, 0);
  for (int64_t p = 0; p < nnz; ++p) f.row_ptr[(size_t)((int64_t)row_idx[p] - base) + 1] += 1;
  for (int64_t i = 0; i < n; ++i) f.row_ptr[(size_t)i + 1] += f.row_ptr[(size_t)i];
  std::vector<int64_t> next(f.row_ptr.begin(), f.row_ptr.end() - 1);
  f.perm.resize((size_t)nnz);
  f.col.resize((size_t)nnz);
  f.val.resize((size_t)nnz);
  for (int64_t p = 0; p < nnz; ++p) {          // ascending p within a row: the sort is stable
    const size_t q = (size_t)next[(size_t)((int64_t)row_idx[p] - base)]++;
    f.col[q] = col_idx[p];
    f.val[q] = vals[p];
    f.perm[q] = p;
  }
  if (base != 0)
    for (int64_t& r : f.row_ptr) r += base;
}
