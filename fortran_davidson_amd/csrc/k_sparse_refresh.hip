// New values on the kept pattern of a sparse operator (dav_update_operator_values, dav_update_operator_values_dev; engine_sparse.hip).
//
// A set call made with dav_keep_value_map on leaves two things with the operator: the VALUE MAP src[q] = p << 1 | mirrored of every
// canonical local entry (CSR) or block (BSR) q - p the position in the caller's vals - and the DIAGONAL SOURCES of the whole matrix, the
// positions of the diagonal entries (diagonal blocks) of every row (block row) in input order behind int64 offsets.  An update then only
// moves values; nothing of the pattern is read or written.  Values are moved, never computed with, and the diagonal is the sum the set
// calls form - from +0.0, in input order - so every bit equals what a fresh set call builds from the same vals.
//
// All kernels: wave64, 256 threads per workgroup, no float atomics, plain vector stores.
//   refresh_csr   val[q] = vals[src[q] >> 1].  A workgroup takes a tile of 2048 consecutive q, a thread 8 of them 256 apart: the src
//                 loads and the val stores of a wave are whole 128-byte segments; the gather in between is nearly monotone for sorted
//                 FULL input and scattered for mirrored entries.  All src loads, then all gathers, are issued before the first store.
//                 24 bytes per local entry (8 map + 8 gathered + 8 stored).  (BSR moves its blocks with bsr_build_gather_kernel.)
//   refresh_diag  one thread per row i of the whole matrix: diag[i] = +0.0 + the entries (m, m), m = i mod b, of the diagonal blocks of
//                 block row i / b in input order; entry (m, m) of block p sits at p b^2 + m b + m in either block layout.  b = 1: CSR.
//   diag_counts   (device set entries) the per-row counts of the check pass widened to int64 behind a leading 0, for the offset scan
//   diag_sources  (device set entries) one thread per row (block row): the positions of its diagonal entries in input order, from the
//                 first one the check pass found, written behind the row's offset
#include "kernels.h"

namespace {
constexpr int SR_THREADS = 256;
constexpr int SR_EPT = 8;                          // entries per thread of the gather
constexpr int SR_TILE = SR_THREADS * SR_EPT;       // entries per workgroup

__global__ __launch_bounds__(SR_THREADS) void sparse_refresh_csr_kernel(const uint64_t* __restrict__ src, int64_t lnnz,
                                                                        const double* __restrict__ vals, double* __restrict__ val) {
  const int64_t tile = (int64_t)blockIdx.x * SR_TILE;
  const int64_t q0 = tile + threadIdx.x;
  uint64_t s[SR_EPT];
  double v[SR_EPT];
  if (tile + SR_TILE <= lnnz) {                                  // a whole tile (uniform over the workgroup)
#pragma unroll
    for (int u = 0; u < SR_EPT; ++u) s[u] = src[q0 + (int64_t)u * SR_THREADS];
#pragma unroll
    for (int u = 0; u < SR_EPT; ++u) v[u] = vals[s[u] >> 1];
#pragma unroll
    for (int u = 0; u < SR_EPT; ++u) val[q0 + (int64_t)u * SR_THREADS] = v[u];
    return;
  }
  // the tail: entries past lnnz are neither read nor written
#pragma unroll
  for (int u = 0; u < SR_EPT; ++u) {
    const int64_t q = q0 + (int64_t)u * SR_THREADS;
    s[u] = q < lnnz ? src[q] : 0;
  }
#pragma unroll
  for (int u = 0; u < SR_EPT; ++u) {
    const int64_t q = q0 + (int64_t)u * SR_THREADS;
    v[u] = q < lnnz ? vals[s[u] >> 1] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < SR_EPT; ++u) {
    const int64_t q = q0 + (int64_t)u * SR_THREADS;
    if (q < lnnz) val[q] = v[u];
  }
}

// B1: a CSR matrix (b = 1, no division)
template <bool B1>
__global__ __launch_bounds__(SR_THREADS) void sparse_refresh_diag_kernel(int b, const int64_t* __restrict__ doff,
                                                                         const int64_t* __restrict__ dpos, const double* __restrict__ vals,
                                                                         int64_t n, double* __restrict__ diag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, bb = (int64_t)b * b;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t I = B1 ? i : i / b;
    const int64_t mm = B1 ? 0 : (i - I * b) * (b + 1);
    const int64_t t1 = doff[I + 1];
    double s = 0.0;
    for (int64_t t = doff[I]; t < t1; ++t) s += vals[B1 ? dpos[t] : dpos[t] * bb + mm];
    diag[i] = s;
  }
}

__global__ __launch_bounds__(SR_THREADS) void sparse_build_diag_counts_kernel(const uint32_t* __restrict__ dcount, int64_t n,
                                                                              int64_t* __restrict__ doff) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) doff[i + 1] = (int64_t)dcount[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) doff[0] = 0;
}

template <class RP, class CI>
__global__ __launch_bounds__(SR_THREADS) void sparse_build_diag_sources_kernel(const RP* __restrict__ rp, const CI* __restrict__ col, int64_t n,
                                                                               int base, const uint32_t* __restrict__ dcount,
                                                                               const unsigned long long* __restrict__ dfirst,
                                                                               const int64_t* __restrict__ doff, int64_t* __restrict__ dpos) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t cnt = dcount[i];
    if (cnt == 0) continue;
    const int64_t p1 = (int64_t)rp[i + 1] - base;
    int64_t t = doff[i];
    uint32_t seen = 0;
    for (int64_t p = (int64_t)dfirst[i]; p < p1 && seen < cnt; ++p)
      if ((int64_t)col[p] - base == i) { dpos[t++] = p; ++seen; }
  }
}

unsigned sr_grid_stride(int64_t items) { return (unsigned)std::min<int64_t>(8192, std::max<int64_t>(1, (items + SR_THREADS - 1) / SR_THREADS)); }
}  // namespace

void launch_sparse_refresh_csr(hipStream_t st, const uint64_t* src, int64_t lnnz, const double* vals, double* val) {
  if (lnnz <= 0) return;
  hipLaunchKernelGGL(sparse_refresh_csr_kernel, dim3((unsigned)((lnnz + SR_TILE - 1) / SR_TILE)), dim3(SR_THREADS), 0, st, src, lnnz, vals, val);
}

int64_t sparse_refresh_tile() { return SR_TILE; }

void launch_sparse_refresh_diag(hipStream_t st, int bs, const int64_t* doff, const int64_t* dpos, const double* vals, int64_t n, double* diag) {
  if (n <= 0) return;
  if (bs == 1) hipLaunchKernelGGL(sparse_refresh_diag_kernel<true>, dim3(sr_grid_stride(n)), dim3(SR_THREADS), 0, st, 1, doff, dpos, vals, n, diag);
  else hipLaunchKernelGGL(sparse_refresh_diag_kernel<false>, dim3(sr_grid_stride(n)), dim3(SR_THREADS), 0, st, bs, doff, dpos, vals, n, diag);
}

void launch_sparse_build_diag_counts(hipStream_t st, const uint32_t* dcount, int64_t n, int64_t* doff) {
  hipLaunchKernelGGL(sparse_build_diag_counts_kernel, dim3(sr_grid_stride(n)), dim3(SR_THREADS), 0, st, dcount, n, doff);
}

void launch_sparse_build_diag_sources(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int base,
                                      const uint32_t* dcount, const unsigned long long* dfirst, const int64_t* doff, int64_t* dpos) {
  if (n <= 0) return;
  cb_dispatch(rp64, ci64, [&](auto r_, auto c_) { using RP = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((sparse_build_diag_sources_kernel<RP, CI>), dim3(sr_grid_stride(n)), dim3(SR_THREADS), 0, st, (const RP*)rp, (const CI*)col, n,
                             base, dcount, dfirst, doff, dpos); });
}
