// Lanczos bound of the Chebyshev-filtered correction of any device operator (DAV_METHOD_LCHEB; engine_cheb.hip): the
// vector work of at most 12 steps of the three-term recurrence on ONE column.  The products A u are the engine's block product, the scalars
// live on the host; this file holds the rest:
//
// lanczos_start    u[i] = (splitmix64(g + 1) >> 11) * 2^-52 - 1 of the global row g = row0 + i (53 bits, exact, in [-1, 1); the same
//                  numbers for any number of ranks), +0.0 into the pad rows, and the partials of <u, u>.
// lanczos_first    the first half of a step from the unnormalised u (|u| = nrm) and au = A u:  v = u / nrm (over u),
//                  w = au / nrm - beta * v_prev (over au; v_prev == nullptr: not read), and the partials of <v, w>.
// lanczos_second   the second half:  w -= alpha * v  and the partials of <w, w>.  This w is the next step's unnormalised u.
// lanczos_finish   one workgroup: the sum of the partials in fixed order into this rank's slot, +0.0 into the slots of the other ranks (the
//                  all-reduce that follows SUMS, x + 0 is exact; the host adds the slots in rank order, so every rank holds the same bits).
//
// Every product and sum is rounded on its own (fp contract off): a restatement in numpy differs only by the order of the dot products.
// Two rows (16 bytes) per lane and array.  A dot product: per lane x + y of its two rows, per wave a __shfl_xor butterfly, per workgroup
// the four waves through LDS in wave order, one partial per workgroup - the grid follows from the rows alone, so the bits do not depend
// on the launch.  wave64, 256 threads, no atomics, plain vector stores.
#include "kernels.h"

namespace {
constexpr int LZ_THREADS = 256;

// the sum over the workgroup, in every thread
__device__ __forceinline__ double lz_block_sum(double s, double* sh) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = s;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < LZ_THREADS / 64; ++w) r += sh[w];
  return r;
}

__global__ __launch_bounds__(LZ_THREADS) void lanczos_start_kernel(double* __restrict__ u, int64_t row0, int64_t nloc, int64_t nrows_pad,
                                                                   double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double sh[LZ_THREADS / 64];
  const int64_t i = 2 * ((int64_t)blockIdx.x * LZ_THREADS + threadIdx.x);
  double s = 0.0;
  if (i < nrows_pad) {
    double2 o = make_double2(0.0, 0.0);
    if (i < nloc) o.x = (double)(dav_splitmix64((uint64_t)(row0 + i) + 1) >> 11) * (1.0 / 4503599627370496.0) - 1.0;
    if (i + 1 < nloc) o.y = (double)(dav_splitmix64((uint64_t)(row0 + i + 1) + 1) >> 11) * (1.0 / 4503599627370496.0) - 1.0;
    *reinterpret_cast<double2*>(u + i) = o;
    const double px = o.x * o.x, py = o.y * o.y;
    s = px + py;
  }
  s = lz_block_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(LZ_THREADS) void lanczos_first_kernel(double* __restrict__ u, double* __restrict__ au, const double* __restrict__ vprev,
                                                                   double nrm, double beta, int64_t nloc, int64_t nrows_pad,
                                                                   double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double sh[LZ_THREADS / 64];
  const int64_t i = 2 * ((int64_t)blockIdx.x * LZ_THREADS + threadIdx.x);
  double s = 0.0;
  if (i < nrows_pad) {
    double2 v = make_double2(0.0, 0.0), w = make_double2(0.0, 0.0);
    if (i < nloc) {
      const double2 uu = *reinterpret_cast<const double2*>(u + i);
      const double2 aa = *reinterpret_cast<const double2*>(au + i);
      double2 vp = make_double2(0.0, 0.0);
      if (vprev) vp = *reinterpret_cast<const double2*>(vprev + i);
      v.x = uu.x / nrm;
      w.x = aa.x / nrm;
      if (vprev) { const double t = beta * vp.x; w.x = w.x - t; }
      if (i + 1 < nloc) {          // an odd nloc: the second row of the pair is the first pad row
        v.y = uu.y / nrm;
        w.y = aa.y / nrm;
        if (vprev) { const double t = beta * vp.y; w.y = w.y - t; }
      }
    }
    *reinterpret_cast<double2*>(u + i) = v;
    *reinterpret_cast<double2*>(au + i) = w;
    const double px = v.x * w.x, py = v.y * w.y;
    s = px + py;
  }
  s = lz_block_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(LZ_THREADS) void lanczos_second_kernel(double* __restrict__ w, const double* __restrict__ v, double alpha, int64_t nloc,
                                                                    int64_t nrows_pad, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double sh[LZ_THREADS / 64];
  const int64_t i = 2 * ((int64_t)blockIdx.x * LZ_THREADS + threadIdx.x);
  double s = 0.0;
  if (i < nrows_pad) {
    double2 o = make_double2(0.0, 0.0);
    if (i < nloc) {
      const double2 ww = *reinterpret_cast<const double2*>(w + i);
      const double2 vv = *reinterpret_cast<const double2*>(v + i);
      const double tx = alpha * vv.x;
      o.x = ww.x - tx;
      if (i + 1 < nloc) {
        const double ty = alpha * vv.y;
        o.y = ww.y - ty;
      }
    }
    *reinterpret_cast<double2*>(w + i) = o;
    const double px = o.x * o.x, py = o.y * o.y;
    s = px + py;
  }
  s = lz_block_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(LZ_THREADS) void lanczos_finish_kernel(const double* __restrict__ partial, int npartial, double* __restrict__ slots,
                                                                    int rank, int nranks) {
  __shared__ double sh[LZ_THREADS / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < npartial; i += LZ_THREADS) s += partial[i];
  const double t = lz_block_sum(s, sh);
  for (int p = threadIdx.x; p < nranks; p += LZ_THREADS) slots[p] = p == rank ? t : 0.0;
}
}  // namespace

int lanczos_partials(int64_t nrows_pad) { return (int)std::max<int64_t>((nrows_pad / 2 + LZ_THREADS - 1) / LZ_THREADS, 1); }

void launch_lanczos_start(hipStream_t st, double* u, int64_t row0, int64_t nloc, int64_t nrows_pad, double* partial, double* slots, int rank,
                          int nranks) {
  const int grid = lanczos_partials(nrows_pad);
  hipLaunchKernelGGL(lanczos_start_kernel, dim3(grid), dim3(LZ_THREADS), 0, st, u, row0, nloc, nrows_pad, partial);
  hipLaunchKernelGGL(lanczos_finish_kernel, dim3(1), dim3(LZ_THREADS), 0, st, partial, grid, slots, rank, nranks);
}

void launch_lanczos_first(hipStream_t st, double* u, double* au, const double* vprev, double nrm, double beta, int64_t nloc, int64_t nrows_pad,
                          double* partial, double* slots, int rank, int nranks) {
  const int grid = lanczos_partials(nrows_pad);
  hipLaunchKernelGGL(lanczos_first_kernel, dim3(grid), dim3(LZ_THREADS), 0, st, u, au, vprev, nrm, beta, nloc, nrows_pad, partial);
  hipLaunchKernelGGL(lanczos_finish_kernel, dim3(1), dim3(LZ_THREADS), 0, st, partial, grid, slots, rank, nranks);
}

void launch_lanczos_second(hipStream_t st, double* w, const double* v, double alpha, int64_t nloc, int64_t nrows_pad, double* partial,
                           double* slots, int rank, int nranks) {
  const int grid = lanczos_partials(nrows_pad);
  hipLaunchKernelGGL(lanczos_second_kernel, dim3(grid), dim3(LZ_THREADS), 0, st, w, v, alpha, nloc, nrows_pad, partial);
  hipLaunchKernelGGL(lanczos_finish_kernel, dim3(1), dim3(LZ_THREADS), 0, st, partial, grid, slots, rank, nranks);
}
