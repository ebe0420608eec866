// Ingest of an initial guess (dav_set_guess, dav_set_guess_dev; engine_guess.hip).
//
// guess_ingest_kernel moves `nrows` rows of `ncols` columns from the caller's array (column-major, leading dimension ldx) into a panel
// (leading dimension ldd), writes +0.0 into the `npad` rows behind them, and in the same pass answers the two questions that decide
// whether the guess is taken: was any entry not finite, and which columns hold a non-zero.  Values are moved as they are, never computed
// with - NaN payloads and signed zeros arrive bit for bit - and the answers are exact: bit tests, no sums, no tolerance.
//
// wave64, 256 threads per workgroup, no inline assembly, no float atomics, plain vector stores.  A workgroup takes one column
// (blockIdx.y) and GI_ROWS consecutive rows of it; a thread GI_UNROLL lanes of V doubles, GI_THREADS lanes apart, so that the loads and
// the stores of a wave are whole contiguous segments (64 x 8 V bytes); all loads of a thread are issued before its first store.
// V = 2 (16-byte lanes) only where the host found both sides 16-byte aligned with even leading dimensions, V = 1 (8-byte lanes)
// otherwise - an odd ldx, a pointer offset by one double: decided per launch, never per element.  With V = 2 the lane that straddles the
// end of the rows (an odd nrows) goes element by element.  Rows past nrows + npad are neither read nor written.
// Flags: each wave folds its lanes with one ballot per question; its first lane then sets the bit with an integer atomic OR (at most two
// per wave).  flags[0] bit 0 = a non-finite entry was seen; flags[1 + c / 64] bit c % 64 = column c holds a non-zero (-0.0 counts as zero).
// 16 bytes per element moved (8 read + 8 written).
#include "kernels.h"

namespace {
constexpr int GI_THREADS = 256;
constexpr int GI_UNROLL = 4;

__device__ __forceinline__ void gi_look(double v, bool& bad, bool& nonzero) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  bad = bad || ((b >> 52) & 0x7ffull) == 0x7ffull;          // Inf or NaN: exponent all ones
  nonzero = nonzero || (b << 1) != 0ull;
}

template <int V>
__global__ __launch_bounds__(GI_THREADS) void guess_ingest_kernel(const double* __restrict__ src, int64_t ldx, int64_t nrows, int64_t npad,
                                                                  double* __restrict__ dst, int64_t ldd, unsigned long long* __restrict__ flags) {
  const int c = (int)blockIdx.y;
  const double* s = src + (int64_t)c * ldx;
  double* d = dst + (int64_t)c * ldd;
  const int64_t r0 = ((int64_t)blockIdx.x * GI_UNROLL * GI_THREADS + threadIdx.x) * V;
  const int64_t rend = nrows + npad;
  double v[GI_UNROLL][V];
  bool bad = false, nonzero = false;
#pragma unroll
  for (int u = 0; u < GI_UNROLL; ++u) {
    const int64_t r = r0 + (int64_t)u * GI_THREADS * V;
    if (V == 2 && r + 1 < nrows) {
      const double2 t = *reinterpret_cast<const double2*>(s + r);
      v[u][0] = t.x; v[u][V - 1] = t.y;
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) v[u][i] = r + i < nrows ? s[r + i] : 0.0;
    }
  }
#pragma unroll
  for (int u = 0; u < GI_UNROLL; ++u) {
    const int64_t r = r0 + (int64_t)u * GI_THREADS * V;
#pragma unroll
    for (int i = 0; i < V; ++i) gi_look(v[u][i], bad, nonzero);        // (the +0.0 of a row past nrows answers neither question)
    if (V == 2 && r + 1 < rend) {
      *reinterpret_cast<double2*>(d + r) = make_double2(v[u][0], v[u][V - 1]);
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i)
        if (r + i < rend) d[r + i] = v[u][i];
    }
  }
  const unsigned long long any_bad = __ballot(bad), any_nonzero = __ballot(nonzero);
  if ((threadIdx.x & 63) == 0) {
    if (any_bad) atomicOr(flags, 1ull);
    if (any_nonzero) atomicOr(flags + 1 + c / 64, 1ull << (c % 64));
  }
}
}  // namespace

int guess_flag_words(int ncols) { return 1 + (ncols + 63) / 64; }

bool guess_ingest_wide(const double* src, int64_t ldx, const double* dst, int64_t ldd) {
  return ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0) && ldx % 2 == 0 && ldd % 2 == 0;
}

void launch_guess_ingest(hipStream_t st, const double* src, int64_t ldx, int64_t nrows, int ncols, int64_t npad, double* dst, int64_t ldd,
                         unsigned long long* flags) {
  if (ncols <= 0 || nrows + npad <= 0) return;
  const bool wide = guess_ingest_wide(src, ldx, dst, ldd);
  const int64_t per_wg = (int64_t)GI_THREADS * GI_UNROLL * (wide ? 2 : 1);
  const dim3 grid((unsigned)((nrows + npad + per_wg - 1) / per_wg), (unsigned)ncols);
  if (wide) hipLaunchKernelGGL(guess_ingest_kernel<2>, grid, dim3(GI_THREADS), 0, st, src, ldx, nrows, npad, dst, ldd, flags);
  else hipLaunchKernelGGL(guess_ingest_kernel<1>, grid, dim3(GI_THREADS), 0, st, src, ldx, nrows, npad, dst, ldd, flags);
}
