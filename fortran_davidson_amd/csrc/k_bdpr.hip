// Block-diagonal preconditioned correction (DAV_METHOD_BDPR; engine_bdpr.hip) of a BSR operator of block size 1 <= b <= 16:
//   T[I b : (I + 1) b, j] = (theta_j B_II - A_II)^-1 R[I b : (I + 1) b, j]       for every local block row I and column j
// with B_II = I for a standard problem - the block-Jacobi form of the scalar DPR rule  t = r / (theta_j B_ii - A_ii)  of k_panel.hip.
//
// bdpr_diag_blocks   the diagonal blocks of the local block rows, b x b column-major each, from the canonical store: one thread per entry
//                    of a block adds that entry of the row's diagonal blocks in stored order (= input order: the sort of a block row is
//                    stable and a mirrored block is never a diagonal one) from +0.0, so the diagonal of the result is OpDesc::diag.
// bdpr_solve<B, GEV> a group of G = 2^ceil(log2 b) consecutive lanes owns the systems of one block row, lane r its row r: the row of
//                    A_II (and B_II) stays in registers over the columns j of the launch's column chunk, the matrices are read once.  Per
//                    column: M = theta_j B_II - A_II entry by entry (the expression of the scalar rule), Gaussian elimination with
//                    partial pivoting on the row of M and the right-hand side held by each lane.  The pivot of step k is the largest
//                    |M[r][k]| among the rows not yet chosen (ties: the lowest row), found with a __shfl_xor butterfly of width G; the
//                    pivot row is broadcast with __shfl from its owner, rows are never swapped; the owner of step k is remembered by the
//                    whole group for the back substitution.  A pivot that is exactly zero gives T = +0.0 for that block and column (the
//                    block form of  den != 0 ? r / den : 0); there is no other guard.  Lanes r >= b of a group are idle rows: never a
//                    pivot, never stored.  The block size is a template parameter (one instantiation per b and problem kind): every loop
//                    over the rows and columns of a block is fully unrolled, so all register arrays are indexed by constants.  The groups of a wave hold consecutive block rows: the loads of R and
//                    the stores of T of a wave are one contiguous segment per column.  The workgroups of the last row chunk also write
//                    +0.0 to the pad rows [nloc, nrows_pad) of their columns.
// wave64, 256 threads per workgroup, no LDS, no atomics, plain vector stores.
#include "kernels.h"

namespace {
constexpr int BD_THREADS = 256;

__global__ __launch_bounds__(BD_THREADS) void bdpr_diag_blocks_kernel(int b, const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                                      const double* __restrict__ val, int64_t nbl, int64_t ib0,
                                                                      double* __restrict__ out) {
  const int64_t bb = (int64_t)b * b, total = nbl * bb, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t I = t / bb, e = t - I * bb;
    const int64_t p1 = rp[I + 1];
    const int32_t want = (int32_t)(ib0 + I);
    double s = 0.0;
    for (int64_t p = rp[I]; p < p1; ++p)
      if (col[p] == want) s += val[p * bb + e];
    out[t] = s;
  }
}

template <int G> __device__ __forceinline__ double bd_bcast(double x, int src) {
  if constexpr (G == 1) return x;
  else return __shfl(x, src, G);
}
constexpr int bd_group(int b) { return b <= 1 ? 1 : b <= 2 ? 2 : b <= 4 ? 4 : b <= 8 ? 8 : 16; }

template <int B, bool GEV>
__global__ __launch_bounds__(BD_THREADS) void bdpr_solve_kernel(const double* __restrict__ dA, const double* __restrict__ dB,
                                                                const double* __restrict__ theta, const double* __restrict__ R, int64_t ldr,
                                                                double* __restrict__ T, int64_t ldt, int ncols, int cols_per_wg, int64_t nbl,
                                                                int64_t nloc, int64_t nrows_pad) {
  constexpr int G = bd_group(B);
  const int r = threadIdx.x & (G - 1);
  const int64_t I = (int64_t)blockIdx.x * (BD_THREADS / G) + threadIdx.x / G;
  const bool live = I < nbl && r < B;               // this lane holds a row of a system
  const int64_t row = I * B + r;
  const int j0 = blockIdx.y * cols_per_wg, j1 = min(ncols, j0 + cols_per_wg);

  double a[B], bm[B];
  const int64_t blk = I * (B * B) + r;
#pragma unroll
  for (int c = 0; c < B; ++c) {
    a[c] = live ? dA[blk + c * B] : 0.0;
    if constexpr (GEV) bm[c] = live ? dB[blk + c * B] : 0.0;
    else bm[c] = c == r ? 1.0 : 0.0;
  }

  for (int j = j0; j < j1; ++j) {
    const double th = theta[j];
    double rhs = live ? R[(int64_t)j * ldr + row] : 0.0;
    double m[B];
#pragma unroll
    for (int c = 0; c < B; ++c) m[c] = fma(th, bm[c], -a[c]);     // th * b - a as the DPR epilogue of k_panel.hip is compiled: one rounding
    bool chosen = r >= B;                            // idle rows are never a pivot
    bool singular = false;
    int own[B];
#pragma unroll
    for (int k = 0; k < B; ++k) {
      // the pivot of column k: largest magnitude among the rows not chosen yet, the lowest row among equals
      double best = chosen ? -1.0 : fabs(m[k]);
      int who = r;
#pragma unroll
      for (int off = 1; off < G; off <<= 1) {
        const double ob = __shfl_xor(best, off, G);
        const int ow = __shfl_xor(who, off, G);
        if (ob > best || (ob == best && ow < who)) { best = ob; who = ow; }
      }
      own[k] = who;
      const double piv = bd_bcast<G>(m[k], who);
      if (piv == 0.0) singular = true;
      const double prhs = bd_bcast<G>(rhs, who);
      const bool elim = !chosen && r != who;
      const double f = elim ? m[k] / piv : 0.0;
#pragma unroll
      for (int c = k + 1; c < B; ++c) {
        const double pc = bd_bcast<G>(m[c], who);
        if (elim) m[c] -= f * pc;
      }
      if (elim) rhs -= f * prhs;
      if (r == who) chosen = true;
    }
    // back substitution: the row chosen at step k holds  m[k] x_k + sum_{c > k} m[c] x_c = rhs
    double t = 0.0;
#pragma unroll
    for (int k = B - 1; k >= 0; --k) {
      const double xk = bd_bcast<G>(rhs / m[k], own[k]);
      rhs -= m[k] * xk;
      if (r == k) t = xk;
    }
    if (singular) t = 0.0;
    if (live) T[(int64_t)j * ldt + row] = t;
  }

  // the pad rows of the written columns
  if (blockIdx.x == gridDim.x - 1)
    for (int j = j0; j < j1; ++j)
      for (int64_t i = nloc + threadIdx.x; i < nrows_pad; i += BD_THREADS) T[(int64_t)j * ldt + i] = 0.0;
}

template <int B>
void bd_launch(hipStream_t st, const double* dA, const double* dB, const double* theta, const double* R, int64_t ldr, double* T, int64_t ldt,
               int ncols, int64_t nbl, int64_t nloc, int64_t nrows_pad) {
  const int64_t per_wg = BD_THREADS / bd_group(B);
  const unsigned gx = (unsigned)std::max<int64_t>(1, (nbl + per_wg - 1) / per_wg);
  // few block rows: the columns are shared out over workgroups as well (about 1024 of them)
  const int ny = (int)std::min<int64_t>(ncols, std::max<int64_t>(1, 1024 / gx));
  const int cols_per_wg = (ncols + ny - 1) / ny;
  const dim3 grid(gx, (unsigned)((ncols + cols_per_wg - 1) / cols_per_wg));
  if (dB) hipLaunchKernelGGL((bdpr_solve_kernel<B, true>), grid, dim3(BD_THREADS), 0, st, dA, dB, theta, R, ldr, T, ldt, ncols, cols_per_wg, nbl, nloc, nrows_pad);
  else hipLaunchKernelGGL((bdpr_solve_kernel<B, false>), grid, dim3(BD_THREADS), 0, st, dA, dB, theta, R, ldr, T, ldt, ncols, cols_per_wg, nbl, nloc, nrows_pad);
}
}  // namespace

void launch_bdpr_diag_blocks(hipStream_t st, int bs, const int64_t* rp, const int32_t* col, const double* val, int64_t nbl, int64_t ib0, double* out) {
  const int64_t total = nbl * bs * bs;
  if (total <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>(8192, (total + BD_THREADS - 1) / BD_THREADS);
  hipLaunchKernelGGL(bdpr_diag_blocks_kernel, dim3(grid), dim3(BD_THREADS), 0, st, bs, rp, col, val, nbl, ib0, out);
}

void launch_bdpr_solve(hipStream_t st, int bs, const double* dA, const double* dB, const double* theta, const double* R, int64_t ldr, double* T,
                       int64_t ldt, int ncols, int64_t nbl, int64_t nloc, int64_t nrows_pad) {
  if (ncols <= 0) return;
  switch (bs) {
#define BD_CASE(B) case B: bd_launch<B>(st, dA, dB, theta, R, ldr, T, ldt, ncols, nbl, nloc, nrows_pad); break;
    BD_CASE(1) BD_CASE(2) BD_CASE(3) BD_CASE(4) BD_CASE(5) BD_CASE(6) BD_CASE(7) BD_CASE(8)
    BD_CASE(9) BD_CASE(10) BD_CASE(11) BD_CASE(12) BD_CASE(13) BD_CASE(14) BD_CASE(15) BD_CASE(16)
#undef BD_CASE
    default: break;          // (the engine has checked 1 <= bs <= 16)
  }
}
