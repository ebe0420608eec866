// Chebyshev-filtered correction (DAV_METHOD_CHEB; engine_cheb.hip) of a sparse operator: for column j with Ritz value theta_j and residue
// r_j the correction is z_d of
//   z_1 = (s_1 / e) r_j,   z_{k+1} = (2 s_{k+1} / e) (A z_k - c z_k + pi_k r_j) - s_k s_{k+1} z_{k-1}
// which equals p_d(A) x_j - p_d(theta_j) x_j for the scaled Chebyshev polynomial p_d of the damped interval [a, b] = [c - e, c + e],
// normalised at a0.  The products A z_k are the engine's block product; this file holds the rest:
//
// cheb_row_bound   b >= the spectral radius: the largest row sum of |a_ij| over the canonical store.  One thread per stored row (CSR) or
//                  per row of a block row (BSR: row m of block row I adds entry (m, k) of its blocks in stored order, k ascending); a row's
//                  sum starts from +0.0 and runs in stored order, so its bits do not depend on the launch.  Maxima: per thread over its
//                  rows, per wave by a __shfl_xor butterfly, per workgroup through LDS, one partial per workgroup; a second one-workgroup
//                  launch takes the maximum of the partials into this rank's slot and writes +0.0 into the slots of the other ranks (the
//                  all-reduce that follows SUMS, x + 0 is exact).  A maximum is independent of the order it is taken in.  NaN propagates.
//                  dia_row_bound: the same for a CSR operator stored by diagonals (k_dia.hip) - one thread per row, its slots added in
//                  ascending offset; a fill slot adds +0.0, so without duplicates the bits are those of the CSR bound.
// cheb_coef        one lane per column: the interval rule from the device copy of theta and the bound, s_k, alpha_k, beta_k (the same in
//                  every lane; lane 0 writes them) and pi_k of the lane's column.  No host round trip between the Ritz values and the steps.
// cheb_step        the recurrence step on panel columns, two rows (16 bytes) per lane and array, arithmetic by cheb_combine (kernels.h):
//                  the same statement the epilogue of the CSR product uses (k_spmm.hip), so the fused and the separate step agree bit
//                  for bit.  The workgroups of the last row chunk write +0.0 to the pad rows.
// wave64, no LDS besides the workgroup maximum, no atomics, plain vector stores.
#include "kernels.h"

namespace {
constexpr int CH_THREADS = 256;

// NaN-propagating maximum: once m is NaN it stays NaN, a NaN x replaces any m
__device__ __forceinline__ double ch_max(double m, double x) { return (x > m || x != x) ? x : m; }

__device__ __forceinline__ double ch_block_max(double m, double* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = ch_max(m, __shfl_xor(m, o, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = m;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < CH_THREADS / 64; ++w) r = ch_max(r, sh[w]);
  return r;
}

__global__ __launch_bounds__(CH_THREADS) void cheb_row_bound_kernel(int b, const int64_t* __restrict__ rp, const double* __restrict__ val,
                                                                    int64_t nbl, double* __restrict__ partial) {
  __shared__ double sh[CH_THREADS / 64];
  const int64_t bb = (int64_t)b * b, total = nbl * b, stride = (int64_t)gridDim.x * blockDim.x;
  double m = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t I = t / b, row = t - I * b;
    const int64_t p1 = rp[I + 1];
    double s = 0.0;
    for (int64_t p = rp[I]; p < p1; ++p)
      for (int k = 0; k < b; ++k) s += __builtin_fabs(val[p * bb + (int64_t)k * b + row]);
    m = ch_max(m, s);
  }
  m = ch_block_max(m, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// an operator stored by diagonals (k_dia.hip): one thread per local row, its slots in ascending offset (coalesced: lane = row)
__global__ __launch_bounds__(CH_THREADS) void dia_row_bound_kernel(const double* __restrict__ dval, int64_t ld, int nd, int64_t nloc,
                                                                   double* __restrict__ partial) {
  __shared__ double sh[CH_THREADS / 64];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double m = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nloc; i += stride) {
    double s = 0.0;
    for (int d = 0; d < nd; ++d) s += __builtin_fabs(dval[(int64_t)d * ld + i]);
    m = ch_max(m, s);
  }
  m = ch_block_max(m, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(CH_THREADS) void cheb_bound_finish_kernel(const double* __restrict__ partial, int npartial, double* __restrict__ slots,
                                                                       int rank, int nranks) {
  __shared__ double sh[CH_THREADS / 64];
  double m = 0.0;
  for (int i = threadIdx.x; i < npartial; i += CH_THREADS) m = ch_max(m, partial[i]);
  m = ch_block_max(m, sh);
  for (int p = threadIdx.x; p < nranks; p += CH_THREADS) slots[p] = p == rank ? m : 0.0;
}

__device__ __forceinline__ bool ch_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }

// The interval: b = the bound, a0 = theta_0, delta = (b - a0) / 64,
//   a = min(max(theta_{min(ncorr, 2 lowest) - 1}, theta_{lowest - 1} + delta), b - delta);   c = (a + b) / 2, e = (b - a) / 2.
// Usable when b and every theta_j, j < ncorr, are finite and a0 < a < b; otherwise coef[CHEB_VALID] = 0 and the steps write +0.0.
__global__ __launch_bounds__(64) void cheb_coef_kernel(const double* __restrict__ theta, int ncorr, int lowest, int degree,
                                                       const double* __restrict__ slots, int nranks, double* __restrict__ coef, int pstride) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 64 + threadIdx.x;
  double b = 0.0;
  for (int p = 0; p < nranks; ++p) b = ch_max(b, slots[p]);
  const double a0 = theta[0];
  bool valid = ch_finite(b) && b > a0;
  for (int i = 0; i < ncorr; ++i) valid = valid && ch_finite(theta[i]);
  const double delta = (b - a0) / 64.0;
  const int iu = (ncorr < 2 * lowest ? ncorr : 2 * lowest) - 1;
  double a = theta[iu];
  const double lo = theta[lowest - 1] + delta, hi = b - delta;
  a = a > lo ? a : lo;
  a = a < hi ? a : hi;
  valid = valid && a > a0 && b > a;
  const double c = (a + b) / 2.0, e = (b - a) / 2.0;
  const double s1 = e / (a0 - c);
  const double th = (j < ncorr ? theta[j] : a0) - c;
  const bool head = j == 0;
  if (head) {
    coef[CHEB_VALID] = valid ? 1.0 : 0.0;
    coef[CHEB_C] = c;
    coef[CHEB_AB] = s1 / e;
    coef[CHEB_AB + 1] = 0.0;
  }
  double sk = s1, pim = 1.0, pik = (s1 / e) * th;         // s_k, pi_{k-1}, pi_k at k = 1
  if (j < ncorr) {
    coef[CHEB_PI + j] = 1.0;
    if (degree > 1) coef[CHEB_PI + pstride + j] = pik;
  }
  for (int k = 1; k < degree; ++k) {
    const double sn = 1.0 / (2.0 / s1 - sk);              // s_{k+1}
    const double alpha = 2.0 * sn / e, beta = sk * sn;
    if (head) { coef[CHEB_AB + 2 * k] = alpha; coef[CHEB_AB + 2 * k + 1] = beta; }
    const double pin = alpha * th * pik - beta * pim;     // pi_{k+1}
    pim = pik; pik = pin; sk = sn;
    if (j < ncorr && k + 1 < degree) coef[CHEB_PI + (int64_t)(k + 1) * pstride + j] = pik;
  }
}

// lane = two consecutive rows of one column; blockIdx.y = column
__global__ __launch_bounds__(CH_THREADS) void cheb_step_kernel(int k, const double* __restrict__ coef, int pstride, const double* __restrict__ az,
                                                               const double* __restrict__ z, const double* __restrict__ r, const double* zprev,
                                                               double* out, int64_t ld, int64_t nloc, int64_t nrows_pad) {
  const int j = blockIdx.y;
  const bool valid = coef[CHEB_VALID] != 0.0;
  const double c = coef[CHEB_C], alpha = coef[CHEB_AB + 2 * k], beta = coef[CHEB_AB + 2 * k + 1];
  const double pi = coef[CHEB_PI + (int64_t)k * pstride + j];
  const int64_t i = 2 * ((int64_t)blockIdx.x * CH_THREADS + threadIdx.x);
  if (i >= nrows_pad) return;
  const int64_t at = (int64_t)j * ld + i;
  double2 o = make_double2(0.0, 0.0);
  if (i < nloc) {
    const double2 rr = *reinterpret_cast<const double2*>(r + at);
    if (k == 0) {
#pragma clang fp contract(off)
      o.x = valid ? alpha * rr.x : 0.0;
      o.y = valid ? alpha * rr.y : 0.0;
    } else {
      const double2 ya = *reinterpret_cast<const double2*>(az + at);
      const double2 zz = *reinterpret_cast<const double2*>(z + at);
      double2 zp = make_double2(0.0, 0.0);
      if (zprev) zp = *reinterpret_cast<const double2*>(zprev + at);
      o.x = cheb_combine(ya.x, zz.x, rr.x, zp.x, zprev != nullptr, c, pi, alpha, beta, valid);
      o.y = cheb_combine(ya.y, zz.y, rr.y, zp.y, zprev != nullptr, c, pi, alpha, beta, valid);
    }
    if (i + 1 >= nloc) o.y = 0.0;        // an odd nloc: the second row of the pair is the first pad row
  }
  *reinterpret_cast<double2*>(out + at) = o;
}
}  // namespace

void launch_cheb_row_bound(hipStream_t st, int bs, const int64_t* rp, const double* val, int64_t nbl, double* partial, double* slots, int rank,
                           int nranks) {
  const int64_t rows = nbl * bs;
  const int grid = (int)std::min<int64_t>(std::max<int64_t>((rows + CH_THREADS - 1) / CH_THREADS, 1), CHEB_BOUND_PARTIALS);
  hipLaunchKernelGGL(cheb_row_bound_kernel, dim3(grid), dim3(CH_THREADS), 0, st, bs, rp, val, nbl, partial);
  hipLaunchKernelGGL(cheb_bound_finish_kernel, dim3(1), dim3(CH_THREADS), 0, st, partial, grid, slots, rank, nranks);
}

void launch_dia_row_bound(hipStream_t st, const double* dval, int64_t ld, int nd, int64_t nloc, double* partial, double* slots, int rank, int nranks) {
  const int grid = (int)std::min<int64_t>(std::max<int64_t>((nloc + CH_THREADS - 1) / CH_THREADS, 1), CHEB_BOUND_PARTIALS);
  hipLaunchKernelGGL(dia_row_bound_kernel, dim3(grid), dim3(CH_THREADS), 0, st, dval, ld, nd, nloc, partial);
  hipLaunchKernelGGL(cheb_bound_finish_kernel, dim3(1), dim3(CH_THREADS), 0, st, partial, grid, slots, rank, nranks);
}

void launch_cheb_coef(hipStream_t st, const double* theta, int ncorr, int lowest, int degree, const double* slots, int nranks, double* coef,
                      int pstride) {
  if (ncorr <= 0) return;
  hipLaunchKernelGGL(cheb_coef_kernel, dim3((ncorr + 63) / 64), dim3(64), 0, st, theta, ncorr, lowest, degree, slots, nranks, coef, pstride);
}

void launch_cheb_step(hipStream_t st, int k, const double* coef, int pstride, const double* az, const double* z, const double* r, const double* zprev,
                      double* out, int64_t ld, int ncols, int64_t nloc, int64_t nrows_pad) {
  if (ncols <= 0 || nrows_pad <= 0) return;
  const dim3 grid((unsigned)((nrows_pad / 2 + CH_THREADS - 1) / CH_THREADS), (unsigned)ncols);
  hipLaunchKernelGGL(cheb_step_kernel, grid, dim3(CH_THREADS), 0, st, k, coef, pstride, az, z, r, zprev, out, ld, nloc, nrows_pad);
}
