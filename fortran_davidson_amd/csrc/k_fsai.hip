// Factorized sparse approximate inverse of C = A - sigma B (davp_build_fsai, engine_fsai.hip; include/davidson_hip_precond.h; DESIGN
// section 29): a sparse lower-triangular G with diag(G C G^T) = 1 on the pattern of tril(A)^level, the power of the lower
// triangle of A.
//
// Everything runs one wave per row, without LDS atomics and without float atomics; the only atomics are integer minima over row numbers
// (the smallest refused row), which give the same answer whatever order the work lands in.
//   pattern1      P_1(i): lanes stride over the sorted canonical row i of A; an entry counts when its column is <= i and differs from the
//                 column before it (duplicates are one column); i itself is appended when the row does not store it.  Ballots give every
//                 lane its slot, so the fill pass writes the columns ascending.
//   pattern_next  P_L(i) = union of P_1(j) over j in P_{L-1}(i).  Every P_1(j) is sorted and holds columns <= j <= i only, so the union is
//                 a merge of at most 64 sorted lists: lane x holds the head of list x, the wave takes the minimum of the heads (the next
//                 column of the union), and every lane whose head equals it moves on.  One step per DISTINCT column - at most 64 for a row
//                 that is kept - and no candidate is ever stored: the 16 KiB of LDS per wave that a sort of the 64 x 64 candidates would
//                 take are not needed, and the result is the sorted, deduplicated list the sort would give.
//   rows          one wave (= one workgroup of 64 threads) per row.  Lane p gathers row p of the lower triangle of C_JJ into LDS by a merge
//                 of the sorted row J_p of A (and of B) against the sorted J; the Cholesky factorisation runs column by column in LDS with
//                 lane p owning row p; the back substitution of L^T y = e_m / l_mm runs from the last row up, y_q broadcast from the lane
//                 that owns it.  Two instances: rows of at most 16 columns (2.2 KiB of LDS per workgroup) and longer ones (33 KiB, four
//                 workgroups per CU); a launch skips the rows of the other class.  Lanes behind m idle: rows do not share a wave.
#include "kernels.h"

namespace {
constexpr int FP_THREADS = 256;
constexpr int FP_WAVES = FP_THREADS / 64;
constexpr int32_t FSAI_NONE = 0x7fffffff;          // head of an exhausted list (n < 2^31: no column reaches it)

__device__ __forceinline__ int32_t fsai_wave_min(int32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

template <bool FILL>
__global__ __launch_bounds__(FP_THREADS) void fsai_pattern1_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col, int64_t n,
                                                                   int64_t* __restrict__ count, const int64_t* __restrict__ prp,
                                                                   int32_t* __restrict__ pcol, unsigned long long* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * FP_WAVES;
  for (int64_t i = (int64_t)blockIdx.x * FP_WAVES + (threadIdx.x >> 6); i < n; i += nwaves) {
    const int64_t a = rp[i], z = rp[i + 1];
    const int64_t out = FILL ? prp[i] : 0;
    const int64_t room = FILL ? prp[i + 1] - out : 0;      // the count pass's answer: a fill never writes behind it
    int64_t total = 0;
    bool diag = false;
    for (int64_t p0 = a; p0 < z; p0 += 64) {               // uniform over the wave
      const int64_t p = p0 + lane;
      bool take = false, past = false;
      int32_t c = 0;
      if (p < z) {
        c = col[p];
        past = (int64_t)c > i;
        take = !past && (p == a || col[p - 1] != c);
      }
      const unsigned long long mask = __ballot(take);
      if (FILL && take) {
        const int64_t slot = total + __popcll(mask & ((1ull << lane) - 1ull));
        if (slot < room) pcol[out + slot] = c;
      }
      diag = diag || __ballot(take && (int64_t)c == i) != 0ull;
      total += __popcll(mask);
      if (__ballot(past) != 0ull) break;                   // the row is sorted: nothing <= i follows
    }
    if (!diag) {
      if (FILL && lane == 0 && total < room) pcol[out + total] = (int32_t)i;
      total += 1;
    }
    if (!FILL && lane == 0) {
      count[i] = total;
      if (total > FSAI_MAX_ROW) atomicMin(bad, (unsigned long long)i);
    }
  }
}

template <bool FILL>
__global__ __launch_bounds__(FP_THREADS) void fsai_pattern_next_kernel(const int64_t* __restrict__ qrp, const int32_t* __restrict__ qcol,
                                                                       const int64_t* __restrict__ p1rp, const int32_t* __restrict__ p1col,
                                                                       int64_t n, int64_t* __restrict__ count, const int64_t* __restrict__ prp,
                                                                       int32_t* __restrict__ pcol, unsigned long long* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * FP_WAVES;
  for (int64_t i = (int64_t)blockIdx.x * FP_WAVES + (threadIdx.x >> 6); i < n; i += nwaves) {
    const int64_t a = qrp[i];
    const int m = (int)min((int64_t)FSAI_MAX_ROW, qrp[i + 1] - a);
    int64_t cur = 0, end = 0;
    if (lane < m) {
      const int64_t j = qcol[a + lane];
      cur = p1rp[j];
      end = p1rp[j + 1];
    }
    int32_t head = cur < end ? p1col[cur] : FSAI_NONE;
    int64_t total = 0;
    int32_t mine = 0;
    for (;;) {                                             // one step per distinct column; uniform over the wave
      const int32_t next = fsai_wave_min(head);
      if (next == FSAI_NONE) break;
      if (FILL && (int64_t)lane == total) mine = next;
      total += 1;
      if (head == next) {
        cur += 1;
        head = cur < end ? p1col[cur] : FSAI_NONE;
      }
    }
    if (FILL) {
      const int64_t out = prp[i], room = prp[i + 1] - out;
      if ((int64_t)lane < total && (int64_t)lane < room) pcol[out + lane] = mine;
    } else if (lane == 0) {
      count[i] = total;
      if (total > FSAI_MAX_ROW) atomicMin(bad, (unsigned long long)i);
    }
  }
}

// lane p: row p of the lower triangle of S_JJ (S = A or B; duplicates summed from +0.0 in stored order) by a merge of the sorted row
// r = J_p of S against J_0 <= ... <= J_p; put(q, sum) takes entry (p, q)
template <class F>
__device__ __forceinline__ void fsai_gather_row(const int64_t* __restrict__ rp, const int32_t* __restrict__ col, const double* __restrict__ val,
                                                int64_t r, const int32_t* J, int p, F&& put) {
  int64_t s = rp[r];
  const int64_t z = rp[r + 1];
  const int32_t first = J[0];
  int64_t hi = z;
  while (s < hi) {                                         // the first entry with a column >= J_0
    const int64_t mid = s + ((hi - s) >> 1);
    if (col[mid] < first) s = mid + 1;
    else hi = mid;
  }
  for (int q = 0; q <= p; ++q) {
    const int32_t c = J[q];
    while (s < z && col[s] < c) ++s;
    double sum = 0.0;
    while (s < z && col[s] == c) { sum += val[s]; ++s; }
    put(q, sum);
  }
}

template <int MAXM>
__global__ __launch_bounds__(64) void fsai_rows_kernel(const int64_t* __restrict__ prp, const int32_t* __restrict__ pcol, int64_t n,
                                                       const int64_t* __restrict__ arp, const int32_t* __restrict__ acol,
                                                       const double* __restrict__ aval, const int64_t* __restrict__ brp,
                                                       const int32_t* __restrict__ bcol, const double* __restrict__ bval, double sigma,
                                                       double* __restrict__ gval, int32_t* __restrict__ grow,
                                                       unsigned long long* __restrict__ bad) {
  constexpr int LD = MAXM + 1;                             // odd: a column of C is read without bank conflicts
  __shared__ double C[MAXM * LD];
  __shared__ int32_t J[MAXM];
  const int lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t a0 = prp[i];
    const int64_t len = prp[i + 1] - a0;
    if (len < 1 || len > MAXM || (MAXM > 16 && len <= 16)) continue;          // the other instance's row (uniform over the workgroup)
    const int m = (int)len;
    __syncthreads();                                       // the row before is done with C and J
    if (lane < m) J[lane] = pcol[a0 + lane];
    __syncthreads();
    if (lane < m) {
      const int64_t r = J[lane];
      double* crow = C + lane * LD;
      fsai_gather_row(arp, acol, aval, r, J, lane, [&](int q, double v) { crow[q] = v; });
      if (brp) fsai_gather_row(brp, bcol, bval, r, J, lane, [&](int q, double v) { crow[q] = crow[q] - sigma * v; });
      else crow[lane] = crow[lane] - sigma * 1.0;
    }
    bool ok = true;
    for (int k = 0; k < m; ++k) {                          // column k of L; m, k and d are uniform over the workgroup
      __syncthreads();
      const double d = C[k * LD + k];
      if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) { ok = false; break; }
      const double l = sqrt(d);
      double lpk = 0.0;
      const bool below = lane > k && lane < m;
      if (below) { lpk = C[lane * LD + k] / l; C[lane * LD + k] = lpk; }
      __syncthreads();
      if (lane == k) C[k * LD + k] = l;
      if (below)
        for (int q = k + 1; q <= lane; ++q) C[lane * LD + q] -= lpk * C[q * LD + k];
    }
    __syncthreads();
    if (!ok) {
      if (lane == 0) atomicMin(bad, (unsigned long long)i);
      continue;
    }
    // L z = e_m has z = e_m / l_mm; L^T y = z from the last row up: y_q = acc_q / l_qq, then acc_p -= l_qp y_q for p < q
    double acc = lane == m - 1 ? 1.0 / C[(m - 1) * LD + (m - 1)] : 0.0;
    double y = 0.0;
    for (int q = m - 1; q >= 0; --q) {
      const double yq = __shfl(acc, q, 64) / C[q * LD + q];
      if (lane == q) y = yq;
      if (lane < q) acc -= C[q * LD + lane] * yq;
    }
    const double ylast = __shfl(y, m - 1, 64);
    if (lane < m) {
      gval[a0 + lane] = y / sqrt(ylast);
      grow[a0 + lane] = (int32_t)i;
    }
  }
}

// info[0] = the longest row of the offsets rp[0..n], info[1] / info[2] = 1 where a row of at most 16 / of more entries exists (all 0
// first): integer maxima, whatever order the workgroups land in
__global__ __launch_bounds__(FP_THREADS) void fsai_row_lengths_kernel(const int64_t* __restrict__ rp, int64_t n,
                                                                      unsigned long long* __restrict__ info) {
  const int64_t stride = (int64_t)gridDim.x * FP_THREADS;
  unsigned long long longest = 0ull, small = 0ull, large = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * FP_THREADS + threadIdx.x; i < n; i += stride) {
    const unsigned long long len = (unsigned long long)(rp[i + 1] - rp[i]);
    longest = max(longest, len);
    if (len <= 16ull) small = 1ull;
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

unsigned fsai_grid(int64_t rows, int per_block) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + per_block - 1) / per_block, 65536)); }
}  // namespace

void launch_fsai_pattern1_count(hipStream_t st, const int64_t* rp, const int32_t* col, int64_t n, int64_t* count, unsigned long long* bad) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fsai_pattern1_kernel<false>, dim3(fsai_grid(n, FP_WAVES)), dim3(FP_THREADS), 0, st, rp, col, n, count, (const int64_t*)nullptr,
                     (int32_t*)nullptr, bad);
}
void launch_fsai_pattern1_fill(hipStream_t st, const int64_t* rp, const int32_t* col, int64_t n, const int64_t* prp, int32_t* pcol) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fsai_pattern1_kernel<true>, dim3(fsai_grid(n, FP_WAVES)), dim3(FP_THREADS), 0, st, rp, col, n, (int64_t*)nullptr, prp, pcol,
                     (unsigned long long*)nullptr);
}
void launch_fsai_pattern_next_count(hipStream_t st, const int64_t* qrp, const int32_t* qcol, const int64_t* p1rp, const int32_t* p1col, int64_t n,
                                    int64_t* count, unsigned long long* bad) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fsai_pattern_next_kernel<false>, dim3(fsai_grid(n, FP_WAVES)), dim3(FP_THREADS), 0, st, qrp, qcol, p1rp, p1col, n, count,
                     (const int64_t*)nullptr, (int32_t*)nullptr, bad);
}
void launch_fsai_pattern_next_fill(hipStream_t st, const int64_t* qrp, const int32_t* qcol, const int64_t* p1rp, const int32_t* p1col, int64_t n,
                                   const int64_t* prp, int32_t* pcol) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fsai_pattern_next_kernel<true>, dim3(fsai_grid(n, FP_WAVES)), dim3(FP_THREADS), 0, st, qrp, qcol, p1rp, p1col, n,
                     (int64_t*)nullptr, prp, pcol, (unsigned long long*)nullptr);
}
void launch_fsai_row_lengths(hipStream_t st, const int64_t* rp, int64_t n, unsigned long long* info) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fsai_row_lengths_kernel, dim3((unsigned)std::min<int64_t>(fsai_grid(n, FP_THREADS), 1024)), dim3(FP_THREADS), 0, st, rp, n, info);
}
void launch_fsai_rows(hipStream_t st, const int64_t* prp, const int32_t* pcol, int64_t n, const int64_t* arp, const int32_t* acol,
                      const double* aval, const int64_t* brp, const int32_t* bcol, const double* bval, double sigma, bool small, bool large,
                      double* gval, int32_t* grow, unsigned long long* bad) {
  if (n <= 0) return;
  if (small)
    hipLaunchKernelGGL(fsai_rows_kernel<16>, dim3(fsai_grid(n, 1)), dim3(64), 0, st, prp, pcol, n, arp, acol, aval, brp, bcol, bval, sigma, gval, grow, bad);
  if (large)
    hipLaunchKernelGGL(fsai_rows_kernel<FSAI_MAX_ROW>, dim3(fsai_grid(n, 1)), dim3(64), 0, st, prp, pcol, n, arp, acol, aval, brp, bcol, bval, sigma, gval,
                       grow, bad);
}
