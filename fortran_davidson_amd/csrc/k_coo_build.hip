// Device build of a CSR operator from COO triples in device memory (davx_set_operator_coo_dev, engine_sparse.hip).
//
// The triples (row_idx[p], col_idx[p], vals[p]), p < nnz < 2^32, come in any order, duplicates included.  Their ROW FORM is the CSR matrix
// of a stable sort by row; the result is what dav_set_operator_csr builds from the row form, bit for bit.  The canonical order of a local
// row is (column, p): for the row form that is (column, offset within the source row), for own entries (column <= row with a lower
// triangle) and mirrored ones (column > row) alike - so the sort key of an entry is  column << 32 | (uint32_t)p,  unique over the matrix.
//
// Passes (wave64, 256 threads per workgroup; integer atomics for counts and slots only, no float atomics):
//   check    entry pass: the first triple that breaks a rule (atomic min over p); entries counted per local row (own, and with
//            DAV_CSR_LOWER the mirror images that land in a local row) and diagonal entries per row of the whole matrix (64-bit counts,
//            written behind a leading 0 so that the scan of k_csr_build.hip turns them into offsets in place)
//   scatter  entry pass: every entry takes an atomic slot of its row (cursor = a copy of the row offsets) and leaves column, tie = p and
//            payload there; a diagonal entry also leaves p in a slot of its row in the DIAGONAL PATTERN (one "row" per matrix row, column
//            0, tie = p, payload = p).  Slot order is whatever the atomics give; the sort that follows removes it - the keys are unique,
//            so every correct sort gives the same arrays.
//   sort     rows of 2..64 entries: coo_sort_small_kernel, one wave per row, key and payload in registers, a bitonic network over
//            cross-lane moves (no LDS allocation, no barrier); four rows per workgroup, grid-stride over the rows.  The network runs over
//            the smallest power of two P >= m lanes only (stages k <= P): a 7-entry row takes 6 exchange steps, a 64-entry row 21.
//            Longer rows go to the LDS sort and the tile/merge path of k_csr_build.hip, unchanged.
//   mark     (DAV_CSR_DIAGONALS) dia_mark of k_dia.hip with the row read from row_idx
// The diagonal is then summed from the sorted diagonal pattern by launch_sparse_refresh_diag (k_sparse_refresh.hip): per row from +0.0 in
// ascending p.  With dav_keep_value_map the payload is the source p << 1 | mirrored and the diagonal pattern stays as doff / dpos.
#include "kernels.h"

namespace {
constexpr int COO_THREADS = 256;
constexpr int COO_EPT = 8;                  // entries per thread of an entry pass (strided by the workgroup: coalesced)
constexpr int COO_SMALL = 64;               // longest row of the in-register sort: one entry per lane
constexpr int COO_WAVES = COO_THREADS / 64;

template <class V> __device__ __forceinline__ V coo_payload(const double* __restrict__ vals, int64_t p, bool mirrored);
template <> __device__ __forceinline__ double coo_payload<double>(const double* __restrict__ vals, int64_t p, bool) { return vals[p]; }
template <> __device__ __forceinline__ uint64_t coo_payload<uint64_t>(const double* __restrict__, int64_t p, bool mirrored) {
  return ((uint64_t)p << 1) | (mirrored ? 1u : 0u);
}

template <class RI, class CI>
__global__ __launch_bounds__(COO_THREADS) void coo_check_kernel(const RI* __restrict__ row, const CI* __restrict__ col, int64_t n, int64_t nnz,
                                                                int base, int lower, int64_t r0, int64_t nloc,
                                                                unsigned long long* __restrict__ first_bad,
                                                                unsigned long long* __restrict__ lcount,
                                                                unsigned long long* __restrict__ dcount) {
  const int64_t tile = (int64_t)blockIdx.x * COO_THREADS * COO_EPT;
  bool found = false;
  for (int k = 0; k < COO_EPT; ++k) {
    const int64_t p = tile + (int64_t)k * COO_THREADS + threadIdx.x;
    if (p >= nnz) break;
    const int64_t i = (int64_t)row[p] - base, j = (int64_t)col[p] - base;
    if (i < 0 || i >= n || j < 0 || j >= n || (lower && j > i)) {
      if (!found) atomicMin(first_bad, (unsigned long long)p);   // the first of this thread (p increases with k)
      found = true;
      continue;
    }
    if (i >= r0 && i < r0 + nloc) atomicAdd(&lcount[i - r0], 1ull);
    if (lower && j < i && j >= r0 && j < r0 + nloc) atomicAdd(&lcount[j - r0], 1ull);
    if (i == j) atomicAdd(&dcount[i], 1ull);
  }
}

// the caller's row and column of triple p (the refusal message of the first offending triple)
template <class RI, class CI>
__global__ void coo_locate_kernel(const RI* __restrict__ row, const CI* __restrict__ col, int64_t p, int64_t* __restrict__ out) {
  out[0] = (int64_t)row[p];
  out[1] = (int64_t)col[p];
}

template <class RI, class CI, class V>
__global__ __launch_bounds__(COO_THREADS) void coo_scatter_kernel(const RI* __restrict__ row, const CI* __restrict__ col,
                                                                  const double* __restrict__ vals, int64_t nnz, int base, int lower,
                                                                  int64_t r0, int64_t nloc, unsigned long long* __restrict__ cursor,
                                                                  int32_t* __restrict__ ocol, V* __restrict__ oval, uint32_t* __restrict__ tie,
                                                                  unsigned long long* __restrict__ dcursor, uint32_t* __restrict__ dtie,
                                                                  uint64_t* __restrict__ dpos) {
  const int64_t tile = (int64_t)blockIdx.x * COO_THREADS * COO_EPT;
  for (int k = 0; k < COO_EPT; ++k) {
    const int64_t p = tile + (int64_t)k * COO_THREADS + threadIdx.x;
    if (p >= nnz) break;
    const int64_t i = (int64_t)row[p] - base, j = (int64_t)col[p] - base;
    if (i >= r0 && i < r0 + nloc) {
      const int64_t q = (int64_t)atomicAdd(&cursor[i - r0], 1ull);
      ocol[q] = (int32_t)j;
      oval[q] = coo_payload<V>(vals, p, false);
      tie[q] = (uint32_t)p;
    }
    if (lower && j < i && j >= r0 && j < r0 + nloc) {
      const int64_t q = (int64_t)atomicAdd(&cursor[j - r0], 1ull);
      ocol[q] = (int32_t)i;
      oval[q] = coo_payload<V>(vals, p, true);
      tie[q] = (uint32_t)p;
    }
    if (i == j) {
      const int64_t q = (int64_t)atomicAdd(&dcursor[i], 1ull);
      dtie[q] = (uint32_t)p;
      dpos[q] = (uint64_t)p;
    }
  }
}

__device__ __forceinline__ uint64_t coo_xor_lane(uint64_t v, int j) { return (uint64_t)__shfl_xor((unsigned long long)v, j, 64); }
__device__ __forceinline__ double coo_xor_lane(double v, int j) { return __shfl_xor(v, j, 64); }

// rows of 2 .. COO_SMALL entries, one wave per row: lane x holds entry x (the lanes behind the row the largest key); after the network
// lane x holds the entry of rank x, and column, payload AND tie are written back in that order - a row left with the ties of its slot
// order would look unsorted to csr_build_flag_kernel wherever it repeats a column, and be sorted again by stale keys.  All branches on m
// and k are uniform over the wave.
template <class V>
__global__ __launch_bounds__(COO_THREADS) void coo_sort_small_kernel(const int64_t* __restrict__ lrp, int64_t nrows, int32_t* __restrict__ ocol,
                                                                     V* __restrict__ oval, uint32_t* __restrict__ tie) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * COO_WAVES;
  for (int64_t i = (int64_t)blockIdx.x * COO_WAVES + (threadIdx.x >> 6); i < nrows; i += nwaves) {
    const int64_t a = lrp[i], len = lrp[i + 1] - a;
    if (len < 2 || len > COO_SMALL) continue;
    const int m = (int)len;
    uint64_t key = ~0ull;
    V val = V{};
    if (lane < m) {
      key = ((uint64_t)(uint32_t)ocol[a + lane] << 32) | tie[a + lane];
      val = oval[a + lane];
    }
#pragma unroll
    for (int k = 2; k <= COO_SMALL; k <<= 1) {
      if ((k >> 1) >= m) break;                       // k > P: the first P lanes are sorted
      const bool up = (lane & k) == 0;
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        const uint64_t okey = coo_xor_lane(key, j);
        const V oval_ = coo_xor_lane(val, j);
        const bool low = (lane & j) == 0;             // the lower lane of the pair keeps the smaller key of an ascending run
        const bool take = (low == up) ? okey < key : okey > key;
        if (take) { key = okey; val = oval_; }
      }
    }
    if (lane < m) {
      ocol[a + lane] = (int32_t)(key >> 32);
      oval[a + lane] = val;
      tie[a + lane] = (uint32_t)key;          // the ties follow their entries: the flag pass of the longer rows reads every row's keys
    }
  }
}

template <class RI, class CI>
__global__ __launch_bounds__(COO_THREADS) void coo_mark_kernel(const RI* __restrict__ row, const CI* __restrict__ col, int64_t n, int64_t nnz,
                                                               int base, int lower, uint8_t* __restrict__ marks,
                                                               unsigned long long* __restrict__ ndiag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned count = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += stride) {
    const int64_t i = (int64_t)row[p] - base, j = (int64_t)col[p] - base;
    marks[j - i + n - 1] = 1;
    if (lower) marks[i - j + n - 1] = 1;
    count += j == i ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) count += __shfl_xor(count, o, 64);
  if ((threadIdx.x & 63) == 0 && count > 0) atomicAdd(ndiag, (unsigned long long)count);
}

unsigned coo_grid(int64_t items, int64_t per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }
}  // namespace

void launch_coo_build_check(hipStream_t st, const void* row, int ri64, const void* col, int ci64, int64_t n, int64_t nnz, int base, int lower,
                            int64_t r0, int64_t nloc, unsigned long long* first_bad, unsigned long long* lcount, unsigned long long* dcount) {
  if (nnz <= 0) return;
  cb_dispatch(ri64, ci64, [&](auto r_, auto c_) { using RI = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((coo_check_kernel<RI, CI>), dim3(coo_grid(nnz, COO_THREADS * COO_EPT)), dim3(COO_THREADS), 0, st,
                             (const RI*)row, (const CI*)col, n, nnz, base, lower, r0, nloc, first_bad, lcount, dcount); });
}

void launch_coo_build_locate(hipStream_t st, const void* row, int ri64, const void* col, int ci64, int64_t p, int64_t* out) {
  cb_dispatch(ri64, ci64, [&](auto r_, auto c_) { using RI = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((coo_locate_kernel<RI, CI>), dim3(1), dim3(1), 0, st, (const RI*)row, (const CI*)col, p, out); });
}

template <class V>
void launch_coo_build_scatter(hipStream_t st, const void* row, int ri64, const void* col, int ci64, const double* vals, int64_t nnz, int base,
                              int lower, int64_t r0, int64_t nloc, unsigned long long* cursor, int32_t* ocol, V* oval, uint32_t* tie,
                              unsigned long long* dcursor, uint32_t* dtie, uint64_t* dpos) {
  if (nnz <= 0) return;
  cb_dispatch(ri64, ci64, [&](auto r_, auto c_) { using RI = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((coo_scatter_kernel<RI, CI, V>), dim3(coo_grid(nnz, COO_THREADS * COO_EPT)), dim3(COO_THREADS), 0, st,
                             (const RI*)row, (const CI*)col, vals, nnz, base, lower, r0, nloc, cursor, ocol, oval, tie, dcursor, dtie, dpos); });
}
template void launch_coo_build_scatter<double>(hipStream_t, const void*, int, const void*, int, const double*, int64_t, int, int, int64_t, int64_t,
                                               unsigned long long*, int32_t*, double*, uint32_t*, unsigned long long*, uint32_t*, uint64_t*);
template void launch_coo_build_scatter<uint64_t>(hipStream_t, const void*, int, const void*, int, const double*, int64_t, int, int, int64_t,
                                                 int64_t, unsigned long long*, int32_t*, uint64_t*, uint32_t*, unsigned long long*, uint32_t*,
                                                 uint64_t*);

template <class V>
void launch_coo_sort_small(hipStream_t st, const int64_t* lrp, int64_t nrows, int32_t* ocol, V* oval, uint32_t* tie) {
  if (nrows <= 0) return;
  hipLaunchKernelGGL(coo_sort_small_kernel<V>, dim3((unsigned)std::min<int64_t>(coo_grid(nrows, COO_WAVES), 65536)), dim3(COO_THREADS), 0, st,
                     lrp, nrows, ocol, oval, tie);
}
template void launch_coo_sort_small<double>(hipStream_t, const int64_t*, int64_t, int32_t*, double*, uint32_t*);
template void launch_coo_sort_small<uint64_t>(hipStream_t, const int64_t*, int64_t, int32_t*, uint64_t*, uint32_t*);

int64_t coo_sort_small_rows() { return COO_SMALL; }

void launch_coo_mark(hipStream_t st, const void* row, int ri64, const void* col, int ci64, int64_t n, int64_t nnz, int base, int lower,
                     uint8_t* marks, unsigned long long* ndiag) {
  if (nnz <= 0) return;
  cb_dispatch(ri64, ci64, [&](auto r_, auto c_) { using RI = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((coo_mark_kernel<RI, CI>), dim3((unsigned)std::min<int64_t>(8192, coo_grid(nnz, COO_THREADS))), dim3(COO_THREADS), 0, st,
                             (const RI*)row, (const CI*)col, n, nnz, base, lower, marks, ndiag); });
}
