// Device build of a BSR operator from the caller's device arrays (dav_set_operator_bsr_dev, engine_sparse.hip): the values.
//
// The index level of a BSR matrix is a CSR pattern over its n / b block rows and is built by the kernels of k_csr_build.hip, which carry
// the SOURCE of every block - input position p and whether the block is mirrored, src = p << 1 | tr - to its canonical place q.  Here the
// 8 b^2 bytes of every block move once:  val[q b^2 + k b + m] = entry (tr ? k : m, tr ? m : k) of input block p  (column-major blocks, a
// mirrored block the transpose of its source).  A row-major own block and a column-major mirrored block are transposed on the way, the
// other two are copied.  Values are moved, never computed with.
//
// gather  one workgroup (256 threads, wave64) per tile of NB consecutive canonical blocks, NB b^2 <= 2048 values.  The tile is read block
//         by block in the caller's order - consecutive lanes read consecutive doubles, whole 128-byte segments wherever a block holds one
//         (b >= 4) - and laid into LDS at the place its element has in the output block, rows padded to an odd length so that the
//         transposing store (lanes b doubles apart) spreads over the banks.  After the barrier the tile is written from LDS as ONE
//         contiguous run of NB b^2 doubles: whole 128-byte segments on the output side for every b.  All loads of a thread are issued
//         before its first LDS store.  b is a template parameter (1..16): every division of the element index is by a constant.
// diag    one thread per row of the matrix: the diagonal blocks of its block row in input order from the first one the check pass found.
// The same two steps for a complex Hermitian CSR matrix, whose values are (re, im) pairs (davh_set_operator_csr_dev): further down.
#include "kernels.h"

namespace {
constexpr int BG_THREADS = 256;
constexpr int BG_VALUES = 2048;             // values of a gather tile (8 per thread)
constexpr int BG_BLOCKS = 512;              // at most that many blocks per tile (b = 1, 2: the block sources are staged in LDS too)

template <int B> struct BgShape {
  static constexpr int BB = B * B;
  static constexpr int NB = BG_VALUES / BB < BG_BLOCKS ? BG_VALUES / BB : BG_BLOCKS;     // blocks per tile
  static constexpr int BP = B | 1;                                                       // padded column length in LDS
  static constexpr int EPT = (NB * BB + BG_THREADS - 1) / BG_THREADS;                    // values per thread
};

template <int B>
__global__ __launch_bounds__(BG_THREADS) void bsr_build_gather_kernel(const uint64_t* __restrict__ src, int64_t lnnzb,
                                                                      const double* __restrict__ vals, int rowmaj,
                                                                      double* __restrict__ val) {
  using S = BgShape<B>;
  constexpr int BB = S::BB, NB = S::NB, BP = S::BP, EPT = S::EPT;
  __shared__ uint64_t ssrc[NB];
  __shared__ double tile[NB * B * BP];
  const int64_t q0 = (int64_t)blockIdx.x * NB;
  const int nbt = (int)(lnnzb - q0 < NB ? lnnzb - q0 : NB);        // blocks of this tile
  const int nval = nbt * BB;
  for (int l = threadIdx.x; l < nbt; l += BG_THREADS) ssrc[l] = src[q0 + l];
  __syncthreads();
  double v[EPT];
  int at[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int e = u * BG_THREADS + threadIdx.x;
    at[u] = -1;
    if (e < nval) {
      const int l = e / BB, r = e - l * BB;
      const uint64_t s = ssrc[l];
      v[u] = vals[(int64_t)(s >> 1) * BB + r];
      const int i = r / B, j = r - i * B;                            // element r of the input block: (i, j) in the caller's layout
      const bool transpose = ((int)(s & 1) != 0) != (rowmaj != 0);   // row-major own, column-major mirrored
      at[u] = l * (B * BP) + (transpose ? j * BP + i : i * BP + j);
    }
  }
#pragma unroll
  for (int u = 0; u < EPT; ++u)
    if (at[u] >= 0) tile[at[u]] = v[u];
  __syncthreads();
  double* __restrict__ out = val + q0 * BB;
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int e = u * BG_THREADS + threadIdx.x;
    if (e < nval) {
      const int l = e / BB, r = e - l * BB;
      const int k = r / B, m = r - k * B;
      out[e] = tile[l * (B * BP) + k * BP + m];
    }
  }
}

template <class RP, class CI>
__global__ __launch_bounds__(BG_THREADS) void bsr_build_diag_kernel(int b, const RP* __restrict__ rp, const CI* __restrict__ col,
                                                                    const double* __restrict__ vals, int64_t nb, int base,
                                                                    const uint32_t* __restrict__ dcount,
                                                                    const unsigned long long* __restrict__ dfirst, double* __restrict__ diag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = nb * b, bb = (int64_t)b * b;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t I = i / b;
    const int64_t mm = (i - I * b) * (b + 1);
    const uint32_t cnt = dcount[I];
    double s = 0.0;
    if (cnt > 0) {
      const int64_t p0 = (int64_t)dfirst[I], p1 = (int64_t)rp[I + 1] - base;
      uint32_t seen = 0;
      for (int64_t p = p0; p < p1 && seen < cnt; ++p)
        if ((int64_t)col[p] - base == I) { s += vals[p * bb + mm]; ++seen; }
    }
    diag[i] = s;
  }
}

// ---- the (re, im) value source (davh_set_operator_csr(_dev)) ------------------------------------------------------------
// Entry p of a complex Hermitian CSR matrix lies in the caller's vals as the pair (a, b) = vals[2 p], vals[2 p + 1] and stands for the
// 2 x 2 block [[a, -b], [b, a]]; a mirrored block is its transpose, the block of conj(h).  The store is that of b = 2: column-major blocks.
//
// gather_pairs  two lanes per canonical block q, lane half h = one column (16 bytes) of the block: val[4 q + 2 h .. + 1] =
//               h == 0 ? (a, tr ? -b : b) : (tr ? b : -b, a).  A wave stores 64 consecutive 16-byte columns (1 KiB, whole 128-byte
//               segments) and reads 32 consecutive sources (256 bytes) and their pairs - consecutive for sorted FULL input, scattered for
//               mirrored entries; the two lanes of a block read the same 16 bytes (one request).  -b is a sign flip: values are moved.
//               All loads of a thread are issued before its first store.  40 bytes per block of this rank besides its 32 stored.
// diag_pairs    one thread per block row I: s = +0.0 + the real parts of its diagonal entries in input order, diag[2 I] = diag[2 I + 1] = s
//               (one 16-byte store).  A diagonal entry whose imaginary part is not +-0.0 (NaN included) is no Hermitian diagonal: the
//               smallest such p goes to *bad by an integer atomicMin (the first per thread is its smallest).
constexpr int BP_EPT = 4;                   // 16-byte columns per thread of gather_pairs
constexpr int BP_TILE = BG_THREADS * BP_EPT;

__global__ __launch_bounds__(BG_THREADS) void bsr_build_gather_pairs_kernel(const uint64_t* __restrict__ src, int64_t lnnzb,
                                                                            const double2* __restrict__ pairs, double2* __restrict__ val) {
  const int64_t t0 = (int64_t)blockIdx.x * BP_TILE + threadIdx.x, total = 2 * lnnzb;
  uint64_t s[BP_EPT];
  double2 z[BP_EPT];
#pragma unroll
  for (int u = 0; u < BP_EPT; ++u) {
    const int64_t t = t0 + (int64_t)u * BG_THREADS;
    s[u] = t < total ? src[t >> 1] : 0;
  }
#pragma unroll
  for (int u = 0; u < BP_EPT; ++u) {
    const int64_t t = t0 + (int64_t)u * BG_THREADS;
    z[u] = t < total ? pairs[s[u] >> 1] : make_double2(0.0, 0.0);
  }
#pragma unroll
  for (int u = 0; u < BP_EPT; ++u) {
    const int64_t t = t0 + (int64_t)u * BG_THREADS;
    if (t >= total) continue;
    const bool tr = (s[u] & 1) != 0, second = (t & 1) != 0;
    const double a = z[u].x, b = z[u].y;
    val[t] = second ? make_double2(tr ? b : -b, a) : make_double2(a, tr ? -b : b);
  }
}

template <class RP, class CI>
__global__ __launch_bounds__(BG_THREADS) void bsr_build_diag_pairs_kernel(const RP* __restrict__ rp, const CI* __restrict__ col,
                                                                          const double2* __restrict__ pairs, int64_t nb, int base,
                                                                          const uint32_t* __restrict__ dcount,
                                                                          const unsigned long long* __restrict__ dfirst,
                                                                          double2* __restrict__ diag, unsigned long long* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; I < nb; I += stride) {
    const uint32_t cnt = dcount[I];
    double s = 0.0;
    if (cnt > 0) {
      const int64_t p0 = (int64_t)dfirst[I], p1 = (int64_t)rp[I + 1] - base;
      uint32_t seen = 0;
      bool clean = true;
      for (int64_t p = p0; p < p1 && seen < cnt; ++p)
        if ((int64_t)col[p] - base == I) {
          const double2 z = pairs[p];
          s += z.x;
          ++seen;
          if (clean && !(z.y == 0.0)) { atomicMin(bad, (unsigned long long)p); clean = false; }
        }
    }
    diag[I] = make_double2(s, s);
  }
}

// the refresh: the same sums and the same check over the kept diagonal sources
__global__ __launch_bounds__(BG_THREADS) void bsr_refresh_diag_pairs_kernel(const int64_t* __restrict__ doff, const int64_t* __restrict__ dpos,
                                                                            const double2* __restrict__ pairs, int64_t nb,
                                                                            double2* __restrict__ diag, unsigned long long* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; I < nb; I += stride) {
    const int64_t t1 = doff[I + 1];
    double s = 0.0;
    bool clean = true;
    for (int64_t t = doff[I]; t < t1; ++t) {
      const int64_t p = dpos[t];
      const double2 z = pairs[p];
      s += z.x;
      if (clean && !(z.y == 0.0)) { atomicMin(bad, (unsigned long long)p); clean = false; }
    }
    diag[I] = make_double2(s, s);
  }
}

template <int B>
void bg_launch(hipStream_t st, const uint64_t* src, int64_t lnnzb, const double* vals, int rowmaj, double* val) {
  constexpr int NB = BgShape<B>::NB;
  hipLaunchKernelGGL(bsr_build_gather_kernel<B>, dim3((unsigned)((lnnzb + NB - 1) / NB)), dim3(BG_THREADS), 0, st, src, lnnzb, vals, rowmaj, val);
}
}  // namespace

void launch_bsr_build_gather(hipStream_t st, int bs, const uint64_t* src, int64_t lnnzb, const double* vals, int rowmaj, double* val) {
  if (lnnzb <= 0) return;
  switch (bs) {
#define BG_CASE(B) case B: bg_launch<B>(st, src, lnnzb, vals, rowmaj, val); break;
    BG_CASE(1) BG_CASE(2) BG_CASE(3) BG_CASE(4) BG_CASE(5) BG_CASE(6) BG_CASE(7) BG_CASE(8)
    BG_CASE(9) BG_CASE(10) BG_CASE(11) BG_CASE(12) BG_CASE(13) BG_CASE(14) BG_CASE(15) BG_CASE(16)
#undef BG_CASE
    default: break;                          // the engine has refused any other block size
  }
}

void launch_bsr_build_gather_pairs(hipStream_t st, const uint64_t* src, int64_t lnnzb, const double* pairs, double* val) {
  if (lnnzb <= 0) return;
  hipLaunchKernelGGL(bsr_build_gather_pairs_kernel, dim3((unsigned)((2 * lnnzb + BP_TILE - 1) / BP_TILE)), dim3(BG_THREADS), 0, st, src, lnnzb,
                     (const double2*)pairs, (double2*)val);
}

void launch_bsr_build_diag_pairs(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, const double* pairs, int64_t nb, int base,
                                 const uint32_t* dcount, const unsigned long long* dfirst, double* diag, unsigned long long* bad) {
  if (nb <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>(8192, (nb + BG_THREADS - 1) / BG_THREADS);
  cb_dispatch(rp64, ci64, [&](auto r_, auto c_) { using RP = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((bsr_build_diag_pairs_kernel<RP, CI>), dim3(grid), dim3(BG_THREADS), 0, st, (const RP*)rp, (const CI*)col,
                             (const double2*)pairs, nb, base, dcount, dfirst, (double2*)diag, bad); });
}

void launch_bsr_refresh_diag_pairs(hipStream_t st, const int64_t* doff, const int64_t* dpos, const double* pairs, int64_t nb, double* diag,
                                   unsigned long long* bad) {
  if (nb <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>(8192, (nb + BG_THREADS - 1) / BG_THREADS);
  hipLaunchKernelGGL(bsr_refresh_diag_pairs_kernel, dim3(grid), dim3(BG_THREADS), 0, st, doff, dpos, (const double2*)pairs, nb, (double2*)diag, bad);
}

void launch_bsr_build_diag(hipStream_t st, int bs, const void* rp, int rp64, const void* col, int ci64, const double* vals, int64_t nb,
                           int base, const uint32_t* dcount, const unsigned long long* dfirst, double* diag) {
  if (nb <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>(8192, (nb * bs + BG_THREADS - 1) / BG_THREADS);
  cb_dispatch(rp64, ci64, [&](auto r_, auto c_) { using RP = decltype(r_); using CI = decltype(c_); hipLaunchKernelGGL((bsr_build_diag_kernel<RP, CI>), dim3(grid), dim3(BG_THREADS), 0, st, bs, (const RP*)rp, (const CI*)col, vals, nb,
                             base, dcount, dfirst, diag); });
}
