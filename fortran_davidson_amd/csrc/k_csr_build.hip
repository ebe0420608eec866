// Device build of a CSR operator from the caller's device arrays (dav_set_operator_csr_dev, engine_sparse.hip).
//
// The result is the canonical storage of the host entry, bit for bit: this rank's rows, own entries first, with DAV_CSR_LOWER the
// mirrored strict lower entries, each row ordered by the key (column, position p in the caller's arrays).  Columns are below 2^31 and a
// row holds fewer than 2^32 entries (the engine refuses longer ones), so the key packs into 64 bits: column << 32 | tie, where tie is the
// entry's offset within its SOURCE row - for an own entry the offset within its own segment, for a mirrored entry (row j, column i) its
// offset within row i.  Rows of the input are contiguous in p, so among the mirrored entries of a row (col, tie) order is p order.
//
// Passes (all wave64, 256 threads per workgroup; no float atomics, integer atomics for counts and positions only):
//   rows     row_ptr[0], row_ptr[n], the first row where row_ptr decreases, the first row of 2^32 or more entries (atomic min)
//   check    entry pass: the first entry that breaks a rule (atomic min); diagonal entries counted per row with their first position;
//            with DAV_CSR_LOWER the mirrored entries counted per local target row
//   lengths  + scan: int64 offsets of the canonical local rows
//   scatter  entry pass: own entries at their place, mirrored entries at atomic slots behind the own segment (tie kept aside)
//   flag     entry pass over the canonical rows: a row whose keys are not increasing
//   sort     flagged rows of at most SORT_TILE entries: one workgroup each, bitonic sort in LDS; longer rows: tiles sorted the same way,
//            then merged in passes (each element finds its place in the other run by a binary search: the keys are unique)
//   diag     the diagonal of the whole matrix: a row's diagonal entries summed in input order from +0.0
// The row of an entry is found by a binary search over row_ptr; consecutive entries of a thread reuse the previous row.
//
// The scatter and the sorts are templates on the 8-byte payload V that travels with a column: the entry's value (double, CSR), or the
// SOURCE of a block (uint64_t: input position p << 1 | mirrored) when the rows are the block rows of a BSR matrix, whose b * b values
// are moved once, after the order is known (dav_set_operator_bsr_dev, k_bsr_build.hip).
#include "kernels.h"

namespace {
constexpr int CB_THREADS = 256;
constexpr int CB_EPT = 8;                   // entries per thread of an entry pass (strided by the workgroup: coalesced)
constexpr int SORT_TILE = 2048;             // entries of a row (or a tile of a long row) sorted in LDS by one workgroup
constexpr int SCAN_EPT = 8;                 // items per thread of the offset scan
constexpr int SCAN_TILE = CB_THREADS * SCAN_EPT;

// largest i in [lo, n) with rp[i] <= P (rp non-decreasing, rp[lo] <= P < rp[n]): the row holding entry position P
template <class RP>
__device__ __forceinline__ int64_t cb_row_of(const RP* __restrict__ rp, int64_t n, int64_t lo, int64_t P) {
  if ((int64_t)rp[lo + 1] > P) return lo;                     // the previous row (the common case of a later entry of a thread)
  if ((int64_t)rp[lo + 2] > P) return lo + 1;
  lo += 2;
  int64_t hi = n - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if ((int64_t)rp[mid] <= P) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ uint64_t cb_key(int32_t c, uint32_t tie) { return ((uint64_t)(uint32_t)c << 32) | tie; }

// what input entry p carries to its canonical place (vals is not read for a block source)
template <class V> __device__ __forceinline__ V cb_payload(const double* __restrict__ vals, int64_t p, bool mirrored);
template <> __device__ __forceinline__ double cb_payload<double>(const double* __restrict__ vals, int64_t p, bool) { return vals[p]; }
template <> __device__ __forceinline__ uint64_t cb_payload<uint64_t>(const double* __restrict__, int64_t p, bool mirrored) {
  return ((uint64_t)p << 1) | (mirrored ? 1u : 0u);
}

template <class RP>
__global__ __launch_bounds__(CB_THREADS) void csr_build_rows_kernel(const RP* __restrict__ rp, int64_t n, unsigned long long* __restrict__ info) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t a = (int64_t)rp[i], b = (int64_t)rp[i + 1];
    if (b < a) atomicMin(&info[0], (unsigned long long)i);
    else if (b - a >= ((int64_t)1 << 32)) atomicMin(&info[3], (unsigned long long)i);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    info[1] = (unsigned long long)(int64_t)rp[0];
    info[2] = (unsigned long long)(int64_t)rp[n];
  }
}

template <class RP, class CI>
__global__ __launch_bounds__(CB_THREADS) void csr_build_check_kernel(const RP* __restrict__ rp, const CI* __restrict__ col, int64_t n,
                                                                     int64_t nnz, int base, int lower, int64_t r0, int64_t nloc,
                                                                     unsigned long long* __restrict__ first_bad, int32_t* __restrict__ mcount,
                                                                     uint32_t* __restrict__ dcount, unsigned long long* __restrict__ dfirst) {
  const int64_t tile = (int64_t)blockIdx.x * CB_THREADS * CB_EPT;
  int64_t row = 0;
  bool found = false;
  for (int k = 0; k < CB_EPT; ++k) {
    const int64_t p = tile + (int64_t)k * CB_THREADS + threadIdx.x;
    if (p >= nnz) break;
    row = cb_row_of(rp, n, row, p + base);
    const int64_t j = (int64_t)col[p] - base;
    if (j < 0 || j >= n || (lower && j > row)) {
      if (!found) atomicMin(first_bad, (unsigned long long)p);   // the first of this thread (p increases with k)
      found = true;
      continue;
    }
    if (j == row) {
      atomicAdd(&dcount[row], 1u);
      atomicMin(&dfirst[row], (unsigned long long)p);
    } else if (lower && j < row && j >= r0 && j < r0 + nloc) {
      atomicAdd(&mcount[j - r0], 1);
    }
  }
}

// the row and the column value of entry p (the refusal message of the first offending entry)
template <class RP, class CI>
__global__ void csr_build_locate_kernel(const RP* __restrict__ rp, const CI* __restrict__ col, int64_t n, int base, int64_t p,
                                        int64_t* __restrict__ out) {
  out[0] = cb_row_of(rp, n, 0, p + base);
  out[1] = (int64_t)col[p];
}

// lrp[i + 1] = own + mirrored entries of local row i (lrp[0] = 0)
template <class RP>
__global__ __launch_bounds__(CB_THREADS) void csr_build_lengths_kernel(const RP* __restrict__ rp, int64_t r0, int64_t nloc,
                                                                       const int32_t* __restrict__ mcount, int64_t* __restrict__ lrp) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nloc; i += stride)
    lrp[i + 1] = (int64_t)rp[r0 + i + 1] - (int64_t)rp[r0 + i] + mcount[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) lrp[0] = 0;
}

// exclusive scan of the 256 thread totals of a workgroup (Hillis-Steele in LDS); returns the sum of the threads before this one
__device__ int64_t cb_block_exclusive(int64_t v, int64_t* sh, int64_t* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < CB_THREADS; off <<= 1) {
    const int64_t add = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int64_t incl = sh[t];
  if (total) *total = sh[CB_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(CB_THREADS) void csr_build_scan_sums_kernel(const int64_t* __restrict__ x, int64_t m, int64_t* __restrict__ sums) {
  __shared__ int64_t sh[CB_THREADS];
  const int64_t b0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_EPT;
  int64_t s = 0;
  for (int u = 0; u < SCAN_EPT; ++u)
    if (b0 + u < m) s += x[b0 + u];
  int64_t total = 0;
  cb_block_exclusive(s, sh, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the tile sums in place
__global__ __launch_bounds__(CB_THREADS) void csr_build_scan_tiles_kernel(int64_t* __restrict__ sums, int64_t nt) {
  __shared__ int64_t sh[CB_THREADS];
  int64_t carry = 0;
  for (int64_t c = 0; c < nt; c += CB_THREADS) {
    const int64_t i = c + threadIdx.x;
    const int64_t v = i < nt ? sums[i] : 0;
    int64_t total = 0;
    const int64_t ex = cb_block_exclusive(v, sh, &total);
    if (i < nt) sums[i] = carry + ex;
    carry += total;
  }
}

// x[0..m) -> inclusive prefix sums, in place
__global__ __launch_bounds__(CB_THREADS) void csr_build_scan_apply_kernel(int64_t* __restrict__ x, int64_t m, const int64_t* __restrict__ sums) {
  __shared__ int64_t sh[CB_THREADS];
  const int64_t b0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_EPT;
  int64_t v[SCAN_EPT];
  int64_t s = 0;
  for (int u = 0; u < SCAN_EPT; ++u) {
    v[u] = b0 + u < m ? x[b0 + u] : 0;
    s += v[u];
  }
  int64_t run = sums[blockIdx.x] + cb_block_exclusive(s, sh, nullptr);
  for (int u = 0; u < SCAN_EPT; ++u) {
    run += v[u];
    if (b0 + u < m) x[b0 + u] = run;
  }
}

// entries [p_lo, p_hi) of the caller's arrays: own entries of local rows to their place, mirrored entries (lower) to an atomic slot of
// their target row behind its own segment; tie (lower only) = offset of the entry within its source row
template <class RP, class CI, class V>
__global__ __launch_bounds__(CB_THREADS) void csr_build_scatter_kernel(const RP* __restrict__ rp, const CI* __restrict__ col,
                                                                       const double* __restrict__ vals, int64_t n, int64_t p_lo, int64_t p_hi,
                                                                       int base, int lower, int64_t r0, int64_t nloc,
                                                                       const int64_t* __restrict__ lrp, int32_t* __restrict__ fill,
                                                                       int32_t* __restrict__ ocol, V* __restrict__ oval,
                                                                       uint32_t* __restrict__ tie) {
  const int64_t tile = p_lo + (int64_t)blockIdx.x * CB_THREADS * CB_EPT;
  int64_t row = 0;
  bool searched = false;
  for (int k = 0; k < CB_EPT; ++k) {
    const int64_t p = tile + (int64_t)k * CB_THREADS + threadIdx.x;
    if (p >= p_hi) break;
    row = searched ? cb_row_of(rp, n, row, p + base) : cb_row_of(rp, n, lower ? 0 : r0, p + base);
    searched = true;
    const int64_t j = (int64_t)col[p] - base;
    const int64_t off = p - ((int64_t)rp[row] - base);
    if (row >= r0 && row < r0 + nloc) {
      const int64_t q = lrp[row - r0] + off;
      ocol[q] = (int32_t)j;
      oval[q] = cb_payload<V>(vals, p, false);
      if (tie) tie[q] = (uint32_t)off;
    }
    if (lower && j < row && j >= r0 && j < r0 + nloc) {
      const int64_t own = (int64_t)rp[j + 1] - (int64_t)rp[j];
      const int64_t q = lrp[j - r0] + own + atomicAdd(&fill[j - r0], 1);
      ocol[q] = (int32_t)row;
      oval[q] = cb_payload<V>(vals, p, true);
      tie[q] = (uint32_t)off;
    }
  }
}

// flag[i] = 1 where the keys of canonical local row i are not increasing (without tie: the own position is the tie)
__global__ __launch_bounds__(CB_THREADS) void csr_build_flag_kernel(const int64_t* __restrict__ lrp, int64_t nloc, int64_t lnnz,
                                                                    const int32_t* __restrict__ ocol, const uint32_t* __restrict__ tie,
                                                                    uint8_t* __restrict__ flag) {
  const int64_t tile = (int64_t)blockIdx.x * CB_THREADS * CB_EPT;
  int64_t row = 0;
  for (int k = 0; k < CB_EPT; ++k) {
    const int64_t q = tile + (int64_t)k * CB_THREADS + threadIdx.x;
    if (q + 1 >= lnnz) break;
    row = cb_row_of(lrp, nloc, row, q);
    if (q + 1 >= lrp[row + 1]) continue;
    const int32_t c0 = ocol[q], c1 = ocol[q + 1];
    const bool bad = tie ? cb_key(c0, tie[q]) > cb_key(c1, tie[q + 1]) : c0 > c1;
    if (bad) flag[row] = 1;
  }
}

__device__ __forceinline__ uint32_t cb_tie(const uint32_t* tie, int64_t q, int64_t a) { return tie ? tie[q] : (uint32_t)(q - a); }

// bitonic sort of m <= SORT_TILE (key, value) pairs in LDS (padded to a power of two with the largest key)
template <class V> __device__ void cb_lds_sort(uint64_t* key, V* val, int m) {
  int P = 64;
  while (P < m) P <<= 1;
  for (int x = m + threadIdx.x; x < P; x += CB_THREADS) { key[x] = ~0ull; val[x] = V{}; }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = threadIdx.x; x < P; x += CB_THREADS) {
        const int l = x ^ j;
        if (l > x) {
          const uint64_t kx = key[x], kl = key[l];
          const bool up = (x & k) == 0;
          if ((kx > kl) == up) {
            key[x] = kl; key[l] = kx;
            const V t = val[x]; val[x] = val[l]; val[l] = t;
          }
        }
      }
      __syncthreads();
    }
}

// flagged rows of at most SORT_TILE entries, one workgroup per row (grid-stride over the local rows), sorted in place
template <class V>
__global__ __launch_bounds__(CB_THREADS) void csr_build_sort_rows_kernel(const int64_t* __restrict__ lrp, int64_t nloc,
                                                                         const uint8_t* __restrict__ flag, int32_t* __restrict__ ocol,
                                                                         V* __restrict__ oval, const uint32_t* __restrict__ tie) {
  __shared__ uint64_t key[SORT_TILE];
  __shared__ V val[SORT_TILE];
  for (int64_t i = blockIdx.x; i < nloc; i += gridDim.x) {
    if (!flag[i]) continue;
    const int64_t a = lrp[i], b = lrp[i + 1];
    if (b - a > SORT_TILE) continue;
    const int m = (int)(b - a);
    for (int x = threadIdx.x; x < m; x += CB_THREADS) {
      key[x] = cb_key(ocol[a + x], cb_tie(tie, a + x, a));
      val[x] = oval[a + x];
    }
    cb_lds_sort(key, val, m);
    for (int x = threadIdx.x; x < m; x += CB_THREADS) {
      ocol[a + x] = (int32_t)(key[x] >> 32);
      oval[a + x] = val[x];
    }
    __syncthreads();
  }
}

// a long row [a, a + m): tile t of SORT_TILE entries sorted into (kout, vout)[t * SORT_TILE ...]
template <class V>
__global__ __launch_bounds__(CB_THREADS) void csr_build_sort_tiles_kernel(int64_t a, int64_t m, const int32_t* __restrict__ ocol,
                                                                          const V* __restrict__ oval, const uint32_t* __restrict__ tie,
                                                                          uint64_t* __restrict__ kout, V* __restrict__ vout) {
  __shared__ uint64_t key[SORT_TILE];
  __shared__ V val[SORT_TILE];
  const int64_t t0 = (int64_t)blockIdx.x * SORT_TILE;
  const int mt = (int)(m - t0 < SORT_TILE ? m - t0 : SORT_TILE);
  for (int x = threadIdx.x; x < mt; x += CB_THREADS) {
    key[x] = cb_key(ocol[a + t0 + x], cb_tie(tie, a + t0 + x, a));
    val[x] = oval[a + t0 + x];
  }
  cb_lds_sort(key, val, mt);
  for (int x = threadIdx.x; x < mt; x += CB_THREADS) {
    kout[t0 + x] = key[x];
    vout[t0 + x] = val[x];
  }
}

// one merge pass over sorted runs of w elements: element x of a run lands at its offset plus the count of smaller keys in the partner run
template <class V>
__global__ __launch_bounds__(CB_THREADS) void csr_build_merge_kernel(int64_t m, int64_t w, const uint64_t* __restrict__ kin,
                                                                     const V* __restrict__ vin, uint64_t* __restrict__ kout,
                                                                     V* __restrict__ vout) {
  const int64_t x = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x;
  if (x >= m) return;
  const int64_t base = x / (2 * w) * (2 * w);
  const bool first = x - base < w;
  const int64_t o0 = first ? base + w : base;                  // the partner run [o0, o1)
  const int64_t o1 = first ? (base + 2 * w < m ? base + 2 * w : m) : base + w;
  const uint64_t k = kin[x];
  int64_t lo = o0, hi = o1;                                    // first index of the partner run with a key > k (keys are unique)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (kin[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  const int64_t dst = base + (x - (first ? base : base + w)) + (lo - o0);
  kout[dst] = k;
  vout[dst] = vin[x];
}

template <class V>
__global__ __launch_bounds__(CB_THREADS) void csr_build_unpack_kernel(int64_t a, int64_t m, const uint64_t* __restrict__ kin,
                                                                      const V* __restrict__ vin, int32_t* __restrict__ ocol,
                                                                      V* __restrict__ oval) {
  const int64_t x = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x;
  if (x >= m) return;
  ocol[a + x] = (int32_t)(kin[x] >> 32);
  oval[a + x] = vin[x];
}

// diag[i] = +0.0 plus the diagonal entries of row i in input order
template <class RP, class CI>
__global__ __launch_bounds__(CB_THREADS) void csr_build_diag_kernel(const RP* __restrict__ rp, const CI* __restrict__ col,
                                                                    const double* __restrict__ vals, int64_t n, int base,
                                                                    const uint32_t* __restrict__ dcount,
                                                                    const unsigned long long* __restrict__ dfirst, double* __restrict__ diag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t cnt = dcount[i];
    double s = 0.0;
    if (cnt > 0) {
      const int64_t p0 = (int64_t)dfirst[i], p1 = (int64_t)rp[i + 1] - base;
      uint32_t seen = 0;
      for (int64_t p = p0; p < p1 && seen < cnt; ++p)
        if ((int64_t)col[p] - base == i) { s += vals[p]; ++seen; }
    }
    diag[i] = s;
  }
}

unsigned cb_grid(int64_t items, int64_t per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }
unsigned cb_grid_stride(int64_t items) { return (unsigned)std::min<int64_t>(8192, cb_grid(items, CB_THREADS)); }
}  // namespace

void launch_csr_build_rows(hipStream_t st, const void* rp, int rp64, int64_t n, unsigned long long* info) {
  cb_dispatch(rp64, 0, [&](auto r_, auto) { using RP = decltype(r_); hipLaunchKernelGGL(csr_build_rows_kernel<RP>, dim3(cb_grid_stride(n)), dim3(CB_THREADS), 0, st, (const RP*)rp, n, info); });
}

void launch_csr_build_check(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int64_t nnz, int base, int lower,
                            int64_t r0, int64_t nloc, unsigned long long* first_bad, int32_t* mcount, uint32_t* dcount,
                            unsigned long long* dfirst) {
  if (nnz <= 0) return;
  cb_dispatch(rp64, ci64, [&](auto r_, auto c_) { using RP = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((csr_build_check_kernel<RP, CI>), dim3(cb_grid(nnz, CB_THREADS * CB_EPT)), dim3(CB_THREADS), 0, st,
                             (const RP*)rp, (const CI*)col, n, nnz, base, lower, r0, nloc, first_bad, mcount, dcount, dfirst); });
}

void launch_csr_build_locate(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int base, int64_t p, int64_t* out) {
  cb_dispatch(rp64, ci64, [&](auto r_, auto c_) { using RP = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((csr_build_locate_kernel<RP, CI>), dim3(1), dim3(1), 0, st, (const RP*)rp, (const CI*)col, n, base, p, out); });
}

void launch_csr_build_offsets(hipStream_t st, const void* rp, int rp64, int64_t r0, int64_t nloc, const int32_t* mcount, int64_t* lrp,
                              int64_t* tile_sums) {
  cb_dispatch(rp64, 0, [&](auto r_, auto) { using RP = decltype(r_); hipLaunchKernelGGL(csr_build_lengths_kernel<RP>, dim3(cb_grid_stride(nloc)), dim3(CB_THREADS), 0, st, (const RP*)rp, r0, nloc,
                                 mcount, lrp); });
  launch_csr_build_scan(st, lrp + 1, nloc, tile_sums);
}

void launch_csr_build_scan(hipStream_t st, int64_t* x, int64_t m, int64_t* tile_sums) {
  if (m <= 0) return;
  const int64_t nt = csr_build_scan_tiles(m);
  hipLaunchKernelGGL(csr_build_scan_sums_kernel, dim3((unsigned)nt), dim3(CB_THREADS), 0, st, x, m, tile_sums);
  hipLaunchKernelGGL(csr_build_scan_tiles_kernel, dim3(1), dim3(CB_THREADS), 0, st, tile_sums, nt);
  hipLaunchKernelGGL(csr_build_scan_apply_kernel, dim3((unsigned)nt), dim3(CB_THREADS), 0, st, x, m, tile_sums);
}

int64_t csr_build_scan_tiles(int64_t m) { return std::max<int64_t>(1, (m + SCAN_TILE - 1) / SCAN_TILE); }

template <class V>
static void cb_scatter(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, const double* vals, int64_t n, int64_t p_lo,
                       int64_t p_hi, int base, int lower, int64_t r0, int64_t nloc, const int64_t* lrp, int32_t* fill, int32_t* ocol, V* oval,
                       uint32_t* tie) {
  if (p_hi <= p_lo) return;
  cb_dispatch(rp64, ci64, [&](auto r_, auto c_) { using RP = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((csr_build_scatter_kernel<RP, CI, V>), dim3(cb_grid(p_hi - p_lo, CB_THREADS * CB_EPT)), dim3(CB_THREADS), 0, st,
                             (const RP*)rp, (const CI*)col, vals, n, p_lo, p_hi, base, lower, r0, nloc, lrp, fill, ocol, oval, tie); });
}

void launch_csr_build_scatter(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, const double* vals, int64_t n, int64_t p_lo,
                              int64_t p_hi, int base, int lower, int64_t r0, int64_t nloc, const int64_t* lrp, int32_t* fill, int32_t* ocol,
                              double* oval, uint32_t* tie) {
  cb_scatter(st, rp, rp64, col, ci64, vals, n, p_lo, p_hi, base, lower, r0, nloc, lrp, fill, ocol, oval, tie);
}

void launch_csr_build_scatter(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int64_t p_lo, int64_t p_hi,
                              int base, int lower, int64_t r0, int64_t nloc, const int64_t* lrp, int32_t* fill, int32_t* ocol, uint64_t* osrc,
                              uint32_t* tie) {
  cb_scatter(st, rp, rp64, col, ci64, (const double*)nullptr, n, p_lo, p_hi, base, lower, r0, nloc, lrp, fill, ocol, osrc, tie);
}

void launch_csr_build_flag(hipStream_t st, const int64_t* lrp, int64_t nloc, int64_t lnnz, const int32_t* ocol, const uint32_t* tie,
                           uint8_t* flag) {
  if (lnnz <= 1 || nloc <= 0) return;
  hipLaunchKernelGGL(csr_build_flag_kernel, dim3(cb_grid(lnnz, CB_THREADS * CB_EPT)), dim3(CB_THREADS), 0, st, lrp, nloc, lnnz, ocol, tie, flag);
}

template <class V>
void launch_csr_build_sort_rows(hipStream_t st, const int64_t* lrp, int64_t nloc, const uint8_t* flag, int32_t* ocol, V* oval,
                                const uint32_t* tie) {
  if (nloc <= 0) return;
  hipLaunchKernelGGL(csr_build_sort_rows_kernel<V>, dim3((unsigned)std::min<int64_t>(nloc, 16384)), dim3(CB_THREADS), 0, st, lrp, nloc, flag,
                     ocol, oval, tie);
}

template <class V>
void launch_csr_build_sort_long(hipStream_t st, int64_t a, int64_t m, int32_t* ocol, V* oval, const uint32_t* tie, uint64_t* k0, V* v0,
                                uint64_t* k1, V* v1) {
  if (m <= 0) return;
  hipLaunchKernelGGL(csr_build_sort_tiles_kernel<V>, dim3(cb_grid(m, SORT_TILE)), dim3(CB_THREADS), 0, st, a, m, ocol, oval, tie, k0, v0);
  for (int64_t w = SORT_TILE; w < m; w *= 2) {
    hipLaunchKernelGGL(csr_build_merge_kernel<V>, dim3(cb_grid(m, CB_THREADS)), dim3(CB_THREADS), 0, st, m, w, k0, v0, k1, v1);
    std::swap(k0, k1);
    std::swap(v0, v1);
  }
  hipLaunchKernelGGL(csr_build_unpack_kernel<V>, dim3(cb_grid(m, CB_THREADS)), dim3(CB_THREADS), 0, st, a, m, k0, v0, ocol, oval);
}

template void launch_csr_build_sort_rows<double>(hipStream_t, const int64_t*, int64_t, const uint8_t*, int32_t*, double*, const uint32_t*);
template void launch_csr_build_sort_rows<uint64_t>(hipStream_t, const int64_t*, int64_t, const uint8_t*, int32_t*, uint64_t*, const uint32_t*);
template void launch_csr_build_sort_long<double>(hipStream_t, int64_t, int64_t, int32_t*, double*, const uint32_t*, uint64_t*, double*, uint64_t*,
                                                 double*);
template void launch_csr_build_sort_long<uint64_t>(hipStream_t, int64_t, int64_t, int32_t*, uint64_t*, const uint32_t*, uint64_t*, uint64_t*,
                                                   uint64_t*, uint64_t*);

int64_t csr_build_sort_tile() { return SORT_TILE; }

void launch_csr_build_diag(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, const double* vals, int64_t n, int base,
                           const uint32_t* dcount, const unsigned long long* dfirst, double* diag) {
  if (n <= 0) return;
  cb_dispatch(rp64, ci64, [&](auto r_, auto c_) { using RP = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((csr_build_diag_kernel<RP, CI>), dim3(cb_grid_stride(n)), dim3(CB_THREADS), 0, st, (const RP*)rp, (const CI*)col,
                             vals, n, base, dcount, dfirst, diag); });
}
