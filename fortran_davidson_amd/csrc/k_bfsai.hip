// Block factorized sparse approximate inverse of C = A - sigma B for BSR operators (davq_build_block_fsai, engine_bfsai.hip;
// include/davidson_hip_bprecond.h): a block lower-triangular G on the pattern of tril(A)^level taken over the BLOCK index
// arrays, with (G C G^T)_II = I_b for every block row I.  The pattern launches are those of k_fsai.hip over the nb block rows; here are
// the cap m b <= 64, the block rows of G and the slots of G^T.
//
//   cap        after a count pass: the smallest block row whose m blocks make more than 64 scalar columns (an integer minimum).
//   rows       one wave (= one workgroup of 64 threads) per block row I.  s = m b scalar columns; lane p = q b + r owns scalar row p of C
//              (row r of block J_q) in LDS with the odd leading dimension of fsai_rows_kernel.  The gather merges the sorted block row J_q
//              of A (and of B) against the sorted J and reads row r of every column-major block, duplicates summed from +0.0 in stored
//              order, of a diagonal block the lower triangle only.  The Cholesky factorisation is the scalar kernel's.  The back
//              substitution L^T X = E (E the last b columns of the identity) keeps its b right-hand sides in registers: one pass from
//              the last row up, column t skipped above its own row.  The block row of G is the last b rows of L^-1; lane p writes
//              X[p][0..b) into block q, the diagonal block's upper triangle as +0.0.  Instances: s <= 16 (2.2 KiB of LDS) and s <= 64
//              (33 KiB, four workgroups per CU), each for b <= 1, 2, 4, 8, 16 right-hand sides.
//   transpose  G holds no duplicate block: a count per block column and a slot per block (integer atomics; the slot order inside a block
//              column is whatever the hardware gives and is removed by the canonical sort of the BSR build that follows), then the
//              blocks copied untouched.  No float atomics anywhere.
#include "kernels.h"

namespace {
constexpr int BF_THREADS = 256;

__global__ __launch_bounds__(BF_THREADS) void bfsai_cap_kernel(const int64_t* __restrict__ count, int64_t nb, int b,
                                                               unsigned long long* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * BF_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * BF_THREADS + threadIdx.x; i < nb; i += stride)
    if (count[i] * b > BFSAI_MAX_COLS) atomicMin(bad, (unsigned long long)i);
}

// info[0] = the longest block row of the offsets rp[0..nb], info[1] / info[2] = 1 where a block row of at most 16 / of more scalar columns
// exists (all 0 first): integer maxima
__global__ __launch_bounds__(BF_THREADS) void bfsai_row_lengths_kernel(const int64_t* __restrict__ rp, int64_t nb, int b,
                                                                       unsigned long long* __restrict__ info) {
  const int64_t stride = (int64_t)gridDim.x * BF_THREADS;
  unsigned long long longest = 0ull, small = 0ull, large = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * BF_THREADS + threadIdx.x; i < nb; i += stride) {
    const unsigned long long len = (unsigned long long)(rp[i + 1] - rp[i]);
    longest = max(longest, len);
    if (len * (unsigned long long)b <= 16ull) small = 1ull;
    else large = 1ull;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    longest = max(longest, (unsigned long long)__shfl_xor(longest, o, 64));
    small |= (unsigned long long)__shfl_xor(small, o, 64);
    large |= (unsigned long long)__shfl_xor(large, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&info[0], longest);
    if (small) atomicMax(&info[1], 1ull);
    if (large) atomicMax(&info[2], 1ull);
  }
}

// lane (q, r): scalar row r of block row R = J_q of S (S = A or B), columns of the blocks J_0 <= ... <= J_q, by a merge of the sorted block
// row against J; entry (r, rr) of a column-major block sits at rr * b + r.  put(p', sum) takes entry (q b + r, p'), p' <= q b + r.
template <class F>
__device__ __forceinline__ void bfsai_gather_row(const int64_t* __restrict__ rp, const int32_t* __restrict__ col, const double* __restrict__ val,
                                                 int b, int64_t R, const int32_t* J, int q, int r, F&& put) {
  const int64_t bb = (int64_t)b * b;
  int64_t s = rp[R];
  const int64_t z = rp[R + 1];
  const int32_t first = J[0];
  int64_t hi = z;
  while (s < hi) {                                         // the first block with a block column >= J_0
    const int64_t mid = s + ((hi - s) >> 1);
    if (col[mid] < first) s = mid + 1;
    else hi = mid;
  }
  for (int qq = 0; qq <= q; ++qq) {
    const int32_t c = J[qq];
    while (s < z && col[s] < c) ++s;
    int64_t s1 = s;
    while (s1 < z && col[s1] == c) ++s1;                   // the duplicates of block (R, c): separate terms in stored order
    const int last = qq == q ? r : b - 1;                  // of the diagonal block the lower triangle only
    for (int rr = 0; rr <= last; ++rr) {
      double sum = 0.0;
      for (int64_t t = s; t < s1; ++t) sum += val[t * bb + (int64_t)rr * b + r];
      put(qq * b + rr, sum);
    }
    s = s1;
  }
}

template <int MAXS, int NB>
__global__ __launch_bounds__(64) void bfsai_rows_kernel(const int64_t* __restrict__ prp, const int32_t* __restrict__ pcol, int64_t nb, int b,
                                                        const int64_t* __restrict__ arp, const int32_t* __restrict__ acol,
                                                        const double* __restrict__ aval, const int64_t* __restrict__ brp,
                                                        const int32_t* __restrict__ bcol, const double* __restrict__ bval, double sigma,
                                                        double* __restrict__ gval, int32_t* __restrict__ grow,
                                                        unsigned long long* __restrict__ bad) {
  constexpr int LD = MAXS + 1;                             // odd: a column of C is read without bank conflicts
  __shared__ double C[MAXS * LD];
  __shared__ int32_t J[MAXS];
  const int lane = threadIdx.x;
  const int64_t bb = (int64_t)b * b;
  for (int64_t i = blockIdx.x; i < nb; i += gridDim.x) {
    const int64_t a0 = prp[i];
    const int64_t len = prp[i + 1] - a0;
    const int64_t cols = len * b;
    if (len < 1 || cols > MAXS || (MAXS > 16 && cols <= 16)) continue;        // the other instance's block row (uniform over the workgroup)
    const int m = (int)len, s = (int)cols;
    __syncthreads();                                       // the block row before is done with C and J
    if (lane < m) J[lane] = pcol[a0 + lane];
    __syncthreads();
    const int q = lane / b, r = lane - q * b;
    if (lane < s) {
      const int64_t R = J[q];
      double* crow = C + lane * LD;
      bfsai_gather_row(arp, acol, aval, b, R, J, q, r, [&](int p, double v) { crow[p] = v; });
      if (brp) bfsai_gather_row(brp, bcol, bval, b, R, J, q, r, [&](int p, double v) { crow[p] = crow[p] - sigma * v; });
      else crow[lane] = crow[lane] - sigma * 1.0;
    }
    bool ok = true;
    for (int k = 0; k < s; ++k) {                          // column k of L; s, k and d are uniform over the workgroup
      __syncthreads();
      const double d = C[k * LD + k];
      if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) { ok = false; break; }
      const double l = sqrt(d);
      double lpk = 0.0;
      const bool below = lane > k && lane < s;
      if (below) { lpk = C[lane * LD + k] / l; C[lane * LD + k] = lpk; }
      __syncthreads();
      if (lane == k) C[k * LD + k] = l;
      if (below)
        for (int p = k + 1; p <= lane; ++p) C[lane * LD + p] -= lpk * C[p * LD + k];
    }
    __syncthreads();
    if (!ok) {
      if (lane == 0) atomicMin(bad, (unsigned long long)i);
      continue;
    }
    // L^T X = E, E = the last b columns of the identity of order s: x[t] of lane p becomes X[p][t].  From the last row up: X[p][t] =
    // x[t] / l_pp in lane p, then x[t] -= l_pj X[p][t] in the lanes j < p.  Column t has nothing above its own row s - b + t.
    double x[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) x[t] = (t < b && lane == s - b + t) ? 1.0 : 0.0;
    for (int p = s - 1; p >= 0; --p) {
      const double lpp = C[p * LD + p];
      const double lpj = lane < p ? C[p * LD + lane] : 0.0;
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        if (t < b && p <= s - b + t) {                     // uniform over the workgroup
          const double xp = __shfl(x[t], p, 64) / lpp;
          if (lane == p) x[t] = xp;
          if (lane < p) x[t] -= lpj * xp;
        }
      }
    }
    // G(I b + t, J_q b + r) = X[q b + r][t]: block q of the block row holds it at t * b + r
    if (lane < s) {
      double* blk = gval + (a0 + q) * bb;
#pragma unroll
      for (int t = 0; t < NB; ++t)
        if (t < b) blk[t * b + r] = (q == m - 1 && r > t) ? 0.0 : x[t];
      if (r == 0) grow[a0 + q] = (int32_t)i;
    }
  }
}

__global__ __launch_bounds__(BF_THREADS) void bfsai_tcount_kernel(const int32_t* __restrict__ pcol, int64_t nnzb,
                                                                  unsigned long long* __restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * BF_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * BF_THREADS + threadIdx.x; p < nnzb; p += stride) atomicAdd(&count[pcol[p]], 1ull);
}

__global__ __launch_bounds__(BF_THREADS) void bfsai_tslot_kernel(const int32_t* __restrict__ pcol, const int32_t* __restrict__ grow, int64_t nnzb,
                                                                 const int64_t* __restrict__ trp, unsigned long long* __restrict__ cursor,
                                                                 int32_t* __restrict__ tcol, int64_t* __restrict__ slot) {
  const int64_t stride = (int64_t)gridDim.x * BF_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * BF_THREADS + threadIdx.x; p < nnzb; p += stride) {
    const int32_t c = pcol[p];
    const int64_t room = trp[c + 1] - trp[c];
    const int64_t k = (int64_t)atomicAdd(&cursor[c], 1ull);
    const int64_t at = k < room ? trp[c] + k : -1;         // the count pass's answer: a slot never lies behind it
    slot[p] = at;
    if (at >= 0) tcol[at] = grow[p];
  }
}

__global__ __launch_bounds__(BF_THREADS) void bfsai_tcopy_kernel(const double* __restrict__ gval, const int64_t* __restrict__ slot, int64_t nnzb,
                                                                 int bb, double* __restrict__ tval) {
  const int64_t stride = (int64_t)gridDim.x * BF_THREADS;
  const int64_t total = nnzb * bb;
  for (int64_t x = (int64_t)blockIdx.x * BF_THREADS + threadIdx.x; x < total; x += stride) {
    const int64_t p = x / bb;
    const int64_t at = slot[p];
    if (at >= 0) tval[at * bb + (x - p * bb)] = gval[x];
  }
}

unsigned bfsai_grid(int64_t work, int per_block) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + per_block - 1) / per_block, 65536)); }

template <int MAXS>
void launch_rows_of(hipStream_t st, const int64_t* prp, const int32_t* pcol, int64_t nb, int b, const int64_t* arp, const int32_t* acol,
                    const double* aval, const int64_t* brp, const int32_t* bcol, const double* bval, double sigma, double* gval, int32_t* grow,
                    unsigned long long* bad) {
  const dim3 grid(bfsai_grid(nb, 1)), block(64);
#define BFSAI_LAUNCH(NB) \
  hipLaunchKernelGGL((bfsai_rows_kernel<MAXS, NB>), grid, block, 0, st, prp, pcol, nb, b, arp, acol, aval, brp, bcol, bval, sigma, gval, grow, bad)
  if (b <= 1) BFSAI_LAUNCH(1);
  else if (b <= 2) BFSAI_LAUNCH(2);
  else if (b <= 4) BFSAI_LAUNCH(4);
  else if (b <= 8) BFSAI_LAUNCH(8);
  else BFSAI_LAUNCH(16);
#undef BFSAI_LAUNCH
}
}  // namespace

void launch_bfsai_cap(hipStream_t st, const int64_t* count, int64_t nb, int b, unsigned long long* bad) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(bfsai_cap_kernel, dim3(std::min(bfsai_grid(nb, BF_THREADS), 1024u)), dim3(BF_THREADS), 0, st, count, nb, b, bad);
}
void launch_bfsai_row_lengths(hipStream_t st, const int64_t* rp, int64_t nb, int b, unsigned long long* info) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(bfsai_row_lengths_kernel, dim3(std::min(bfsai_grid(nb, BF_THREADS), 1024u)), dim3(BF_THREADS), 0, st, rp, nb, b, info);
}
void launch_bfsai_rows(hipStream_t st, const int64_t* prp, const int32_t* pcol, int64_t nb, int b, const int64_t* arp, const int32_t* acol,
                       const double* aval, const int64_t* brp, const int32_t* bcol, const double* bval, double sigma, bool small, bool large,
                       double* gval, int32_t* grow, unsigned long long* bad) {
  if (nb <= 0 || b < 1 || b > 16) return;
  if (small) launch_rows_of<16>(st, prp, pcol, nb, b, arp, acol, aval, brp, bcol, bval, sigma, gval, grow, bad);
  if (large) launch_rows_of<BFSAI_MAX_COLS>(st, prp, pcol, nb, b, arp, acol, aval, brp, bcol, bval, sigma, gval, grow, bad);
}
void launch_bfsai_transpose_count(hipStream_t st, const int32_t* pcol, int64_t nnzb, int64_t* count) {
  if (nnzb <= 0) return;
  hipLaunchKernelGGL(bfsai_tcount_kernel, dim3(std::min(bfsai_grid(nnzb, BF_THREADS), 4096u)), dim3(BF_THREADS), 0, st, pcol, nnzb,
                     (unsigned long long*)count);
}
void launch_bfsai_transpose_fill(hipStream_t st, const int32_t* pcol, const int32_t* grow, const double* gval, int64_t nnzb, int b,
                                 const int64_t* trp, int64_t* cursor, int64_t* slot, int32_t* tcol, double* tval) {
  if (nnzb <= 0) return;
  hipLaunchKernelGGL(bfsai_tslot_kernel, dim3(std::min(bfsai_grid(nnzb, BF_THREADS), 4096u)), dim3(BF_THREADS), 0, st, pcol, grow, nnzb, trp,
                     (unsigned long long*)cursor, tcol, slot);
  hipLaunchKernelGGL(bfsai_tcopy_kernel, dim3(std::min(bfsai_grid(nnzb * b * b, BF_THREADS), 8192u)), dim3(BF_THREADS), 0, st, gval, slot, nnzb,
                     b * b, tval);
}
