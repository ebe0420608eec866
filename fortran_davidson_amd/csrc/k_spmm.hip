// K1c: block product of a CSR operator, Y[rows of this rank, 0:kk] = A_csr * X (dav_set_operator_csr).
//
// X arrives in the packed operand of the row-slab path (launch_pack_xt, all-gathered over the ranks): xt[g][j * 16 + c] = X[j, 16 g + c],
// so the 16 columns of group g of row j are one contiguous 128-byte segment.  One wave per work item (kernels.h: CsrItem); its 64 lanes
// are (stream s, group g, column c) with GP = 1, 2 or 4 column groups and S = 4 / GP streams: stream s takes the entries s, s + S,
// s + 2 S, ... of a row (or chunk), each lane one column, so a wave reads S consecutive (column index, value) pairs per step and, for
// each of them, GP whole 128-byte segments of X.  Every stream sums its entries in order; the S stream sums are added in stream order;
// the chunks of a long row are added in chunk order by the finishing pass.  No atomics: the bits of a row depend on its canonical
// entries, CSR_CHUNK and GP only - not on the rank count, the work list or the launch.
//
// Results of whole rows are staged in LDS ([row][column], one region of 16 GP columns per wave: 2 / 4 / 8 KiB) and stored column by
// column: 16 consecutive rows of a panel column (128 bytes) per quarter-wave.  Partial rows of chunks go to part[slot][0:64] (one
// 512-byte row per chunk).
//
// EPI = ChebEpi (launch_spmm_csr_cheb / launch_spmm_csr_finish_cheb): the two places that store a finished row value - the
// column-by-column store from LDS and the finishing pass of the long rows - store cheb_combine (kernels.h) of it instead, the step of the
// Chebyshev correction, so that the product is never written and read back.  The epilogue is a trailing argument pack: empty for the plain
// product, whose kernels keep their signature, their instructions and their order of summation.
#include "kernels.h"

namespace {
constexpr int SPMM_UNROLL = 8;          // steps of a stream whose loads are issued before their FMAs
}

namespace {
__device__ __forceinline__ double spmm_epilogue(double y, int64_t row, int col, const ChebEpi& epi) {
  const int64_t at = (int64_t)col * epi.ld + row;
  return cheb_combine(y, epi.z[at], epi.r[at], epi.zprev ? epi.zprev[at] : 0.0, epi.zprev != nullptr, epi.hdr[CHEB_C], epi.pi[col], epi.ab[0],
                      epi.ab[1], epi.hdr[CHEB_VALID] != 0.0);
}
}  // namespace

template <int GP, class... EPI>
__global__ __launch_bounds__(256) void spmm_csr_kernel(const CsrItem* __restrict__ items, int nitems, const int64_t* __restrict__ rp,
                                                       const int32_t* __restrict__ col, const double* __restrict__ val,
                                                       const double* __restrict__ xt, int64_t gstride, int kk, double* __restrict__ part,
                                                       double* __restrict__ dst, int64_t ldd, EPI... epi) {
  constexpr int S = 4 / GP;
  constexpr int LD = 16 * GP + 1;       // staging row of the launch's columns, padded: a column read by 16 rows hits 16 different banks
  __shared__ double stage[4][CSR_ROWS][LD];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = (lane >> 4) % GP, s = (lane >> 4) / GP;
  const int it = blockIdx.x * 4 + wave;
  int64_t p0 = 0, p1 = 0;
  int row = 0, nrows = 0, slot = -1;
  if (it < nitems) {
    const CsrItem item = items[it];
    p0 = item.p0; p1 = item.p1; row = item.row; nrows = item.nrows; slot = item.slot;
  }
  const double* __restrict__ xg = xt + (int64_t)g * gstride + c;
  for (int r = 0; r < nrows; ++r) {
    const int64_t a = slot >= 0 ? p0 : rp[row + r];
    const int64_t b = slot >= 0 ? p1 : rp[row + r + 1];
    double acc = 0.0;
    for (int64_t p = a + s; p < b; p += (int64_t)S * SPMM_UNROLL) {
      int j[SPMM_UNROLL];
      double v[SPMM_UNROLL], x[SPMM_UNROLL];
#pragma unroll
      for (int u = 0; u < SPMM_UNROLL; ++u) {
        const int64_t q = p + (int64_t)u * S;
        j[u] = q < b ? col[q] : 0;
        v[u] = q < b ? val[q] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < SPMM_UNROLL; ++u) x[u] = xg[(int64_t)j[u] * 16];
#pragma unroll
      for (int u = 0; u < SPMM_UNROLL; ++u)
        if (p + (int64_t)u * S < b) acc = __builtin_fma(v[u], x[u], acc);
    }
    // stream sums in stream order, into the lanes of stream 0 (lane = output column)
    double tot = acc;
#pragma unroll
    for (int q = 1; q < S; ++q) tot += __shfl(acc, (lane + 16 * GP * q) & 63, 64);
    if (s == 0) {
      if (slot >= 0) part[(int64_t)slot * 64 + lane] = tot;
      else stage[wave][r][lane] = tot;
    }
  }
  __syncthreads();
  if (slot >= 0) return;
  // column-major store of the staged rows: lane = (column offset cc, row rr), 16 consecutive rows of 4 columns per instruction
  const int rr = lane & 15, cc = lane >> 4;
  if (rr < nrows) {
    if constexpr (sizeof...(EPI) > 0) {
      for (int cl = cc; cl < kk; cl += 4) dst[(int64_t)cl * ldd + row + rr] = spmm_epilogue(stage[wave][rr][cl], row + rr, cl, epi...);
    } else {
      for (int cl = cc; cl < kk; cl += 4) dst[(int64_t)cl * ldd + row + rr] = stage[wave][rr][cl];
    }
  }
}

// one wave per long row: lane = column, the row's chunk partials added in chunk order (loads issued SPMM_UNROLL chunks ahead of the
// adds: the arrowhead row of N = 10^6 has 977 chunks, and one dependent load per chunk made this wave the tail of the apply)
template <class... EPI>
__global__ __launch_bounds__(64) void spmm_csr_finish_kernel(const CsrLong* __restrict__ longs, const double* __restrict__ part, int kk,
                                                             double* __restrict__ dst, int64_t ldd, EPI... epi) {
  const CsrLong L = longs[blockIdx.x];
  const int lane = threadIdx.x;
  const double* __restrict__ pp = part + (int64_t)L.first * 64 + lane;
  double sum = pp[0];
  int q = 1;
  for (; q + SPMM_UNROLL <= L.count; q += SPMM_UNROLL) {
    double v[SPMM_UNROLL];
#pragma unroll
    for (int u = 0; u < SPMM_UNROLL; ++u) v[u] = pp[(int64_t)(q + u) * 64];
#pragma unroll
    for (int u = 0; u < SPMM_UNROLL; ++u) sum += v[u];
  }
  for (; q < L.count; ++q) sum += pp[(int64_t)q * 64];
  if (lane < kk) {
    if constexpr (sizeof...(EPI) > 0) sum = spmm_epilogue(sum, L.row, lane, epi...);
    dst[(int64_t)lane * ldd + L.row] = sum;
  }
}

namespace {
template <class... EPI>
void spmm_csr_launch(hipStream_t st, const CsrItem* items, int nitems, const int64_t* rp, const int32_t* col, const double* val, const double* xt,
                     int64_t xt_gstride, int groups, int kk, double* part, double* dst, int64_t ldd, EPI... epi) {
  if (nitems <= 0 || kk <= 0) return;
  const dim3 grid((unsigned)((nitems + 3) / 4)), block(256);
  if (groups == 1)
    hipLaunchKernelGGL((spmm_csr_kernel<1, EPI...>), grid, block, 0, st, items, nitems, rp, col, val, xt, xt_gstride, kk, part, dst, ldd, epi...);
  else if (groups == 2)
    hipLaunchKernelGGL((spmm_csr_kernel<2, EPI...>), grid, block, 0, st, items, nitems, rp, col, val, xt, xt_gstride, kk, part, dst, ldd, epi...);
  else
    hipLaunchKernelGGL((spmm_csr_kernel<4, EPI...>), grid, block, 0, st, items, nitems, rp, col, val, xt, xt_gstride, kk, part, dst, ldd, epi...);
}
}  // namespace

void launch_spmm_csr(hipStream_t st, const CsrItem* items, int nitems, const int64_t* rp, const int32_t* col, const double* val,
                     const double* xt, int64_t xt_gstride, int groups, int kk, double* part, double* dst, int64_t ldd) {
  spmm_csr_launch(st, items, nitems, rp, col, val, xt, xt_gstride, groups, kk, part, dst, ldd);
}

void launch_spmm_csr_cheb(hipStream_t st, const CsrItem* items, int nitems, const int64_t* rp, const int32_t* col, const double* val,
                          const double* xt, int64_t xt_gstride, int groups, int kk, double* part, double* dst, int64_t ldd, const ChebEpi& epi) {
  spmm_csr_launch<ChebEpi>(st, items, nitems, rp, col, val, xt, xt_gstride, groups, kk, part, dst, ldd, epi);
}

void launch_spmm_csr_finish(hipStream_t st, const CsrLong* longs, int nlong, const double* part, int kk, double* dst, int64_t ldd) {
  if (nlong <= 0 || kk <= 0) return;
  hipLaunchKernelGGL(spmm_csr_finish_kernel<>, dim3((unsigned)nlong), dim3(64), 0, st, longs, part, kk, dst, ldd);
}

void launch_spmm_csr_finish_cheb(hipStream_t st, const CsrLong* longs, int nlong, const double* part, int kk, double* dst, int64_t ldd,
                                 const ChebEpi& epi) {
  if (nlong <= 0 || kk <= 0) return;
  hipLaunchKernelGGL(spmm_csr_finish_kernel<ChebEpi>, dim3((unsigned)nlong), dim3(64), 0, st, longs, part, kk, dst, ldd, epi);
}
