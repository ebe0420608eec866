// K1d: a CSR operator stored by diagonals (DAV_CSR_DIAGONALS; engine_sparse.hip): the marks of its offsets, the fill of its slots and
// the block product Y[rows of this rank, 0:kk] = A * X.
//
// Storage per rank: off[0..nd), the sorted offsets column - row of the WHOLE matrix, and val[d][i], the entry (row0 + i, row0 + i + off[d])
// of local row i, fp64, leading dimension ld = nloc rounded up to 16 (every diagonal starts on a 128-byte boundary).  A slot without a
// stored entry, or whose column falls outside [0, n), holds +0.0; duplicates of a position are added into their slot from +0.0 in
// canonical order.  A fill slot is multiplied like any other: a non-finite entry of X can reach rows whose stored pattern does not touch it.
//
// dia_mark   (device entry) one thread per entry of the caller's arrays: mark[column - row + n - 1] = 1, with DAV_CSR_LOWER the mirror
//            image too (byte stores of the same value); the diagonal entries are counted (integer atomic, one per wave).  The host entry
//            fills the same table in dia_rule.h.
// dia_fill   one thread per local row (and per pad row of ld): its nd slots are written +0.0, then the row's canonical entries are walked
//            in order - equal columns are neighbours, their values are added from +0.0 - and each sum is stored at the slot that a binary
//            search over off finds.  Plain stores, no atomics; the same thread writes a slot twice, in program order.
// spmm_dia   the product.  X arrives in the packed operand of the row-slab path, xt[g][j * 16 + c] = X[j, 16 g + c].  A workgroup of four
//            waves owns DIA_TILE = 64 consecutive local rows, a wave 16 of them as four strips of 4 rows; a lane is (row rr of the strip,
//            column c) and holds one accumulator per strip and column group (GP = 1, 2 or 4).  For one diagonal and strip a wave reads, per
//            column group, rows i + off .. i + off + 3 of xt: 512 contiguous bytes, no index, no gather.  The values of DIA_CHUNK diagonals
//            of the tile are fetched by coalesced loads (512 bytes per wave and diagonal; the next chunk's are in flight during this
//            chunk's FMAs) and staged in LDS, where a wave reads 4 different addresses per strip.  The offsets are uniform: scalar loads.
//            The loads of DIA_UNROLL diagonals are issued before their FMAs.  A row + off outside [0, n) reads the clamped row 0 or n - 1
//            of xt (its slot is +0.0); the rows behind nloc of the last tile read row nloc - 1: no lane forms an address outside the
//            operand.  ORDER: one accumulator per (row, column), acc = fma(val, x, acc) over the diagonals in ascending offset from +0.0,
//            no split into streams - the bits of a row depend on the matrix alone, not on the rank count, the tile, the launch or the
//            block width.  An accumulator that starts at +0.0 never becomes -0.0 under round-to-nearest (x + (-x) and +0 + (-0) are +0),
//            so a fill slot - fma(+0.0, x, acc) = acc for finite x - does not change a bit.  Results are staged in LDS ([row][column],
//            padded) and stored column by column, 16 consecutive rows (128 bytes) per quarter wave.  EPI = ChebEpi: the one store of a
//            finished value stores cheb_combine of it (the fused step of the Chebyshev correction, as in k_spmm.hip).
// Traffic model of one product (dav_stats): apply_bytes = 8 nd nloc + 4 nd + 8 N k + 8 nloc k (the slots, the offsets, the gathered
// operand once, the rows written; the epilogue's reads on top), apply_flops = 2 k x the canonical entries of this rank (the useful work,
// comparable with the CSR figure; the FMAs executed are nd nloc k).
// wave64, no inline assembly, no atomics outside dia_mark's count, plain vector stores.
#include "kernels.h"

namespace {
constexpr int DIA_TILE = 64;            // rows of a workgroup
constexpr int DIA_CHUNK = 16;           // diagonals staged in LDS per step
constexpr int DIA_UNROLL = 8;           // diagonals whose loads are issued before their FMAs
constexpr int DIA_THREADS = 256;

template <class RP>
__device__ __forceinline__ int64_t dia_row_of(const RP* __restrict__ rp, int64_t n, int64_t P) {      // largest i with rp[i] <= P
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if ((int64_t)rp[mid] <= P) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <class RP, class CI>
__global__ __launch_bounds__(DIA_THREADS) void dia_mark_kernel(const RP* __restrict__ rp, const CI* __restrict__ col, int64_t n, int64_t nnz,
                                                               int base, int lower, uint8_t* __restrict__ marks,
                                                               unsigned long long* __restrict__ ndiag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned count = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += stride) {
    const int64_t i = dia_row_of(rp, n, p + base);
    const int64_t j = (int64_t)col[p] - base;
    marks[j - i + n - 1] = 1;
    if (lower) marks[i - j + n - 1] = 1;
    count += j == i ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) count += __shfl_xor(count, o, 64);
  if ((threadIdx.x & 63) == 0 && count > 0) atomicAdd(ndiag, (unsigned long long)count);
}

__global__ __launch_bounds__(DIA_THREADS) void dia_fill_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                               const double* __restrict__ val, int64_t nloc, int64_t row0,
                                                               const int32_t* __restrict__ off, int nd, double* __restrict__ dval, int64_t ld) {
  const int64_t i = (int64_t)blockIdx.x * DIA_THREADS + threadIdx.x;
  if (i >= ld) return;
  for (int d = 0; d < nd; ++d) dval[(int64_t)d * ld + i] = 0.0;
  if (i >= nloc) return;
  const int64_t z = rp[i + 1];
  int64_t p = rp[i];
  while (p < z) {
    const int32_t cj = col[p];
    double sum = 0.0;
    for (; p < z && col[p] == cj; ++p) sum += val[p];
    const int64_t want = (int64_t)cj - (row0 + i);
    int lo = 0, hi = nd - 1;
    while (lo < hi) {
      const int mid = (lo + hi) / 2;
      if ((int64_t)off[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    if (nd > 0 && (int64_t)off[lo] == want) dval[(int64_t)lo * ld + i] = sum;
  }
}

// (the statement of k_spmm.hip's epilogue, repeated here so that the CSR kernels' file stays as it is)
__device__ __forceinline__ double dia_epilogue(double y, int64_t row, int col, const ChebEpi& epi) {
  const int64_t at = (int64_t)col * epi.ld + row;
  return cheb_combine(y, epi.z[at], epi.r[at], epi.zprev ? epi.zprev[at] : 0.0, epi.zprev != nullptr, epi.hdr[CHEB_C], epi.pi[col], epi.ab[0],
                      epi.ab[1], epi.hdr[CHEB_VALID] != 0.0);
}

template <int GP, class... EPI>
__global__ __launch_bounds__(DIA_THREADS) void spmm_dia_kernel(const int32_t* __restrict__ off, int nd, const double* __restrict__ dval, int64_t ld,
                                                               int64_t nloc, int64_t row0, int64_t n, const double* __restrict__ xt,
                                                               int64_t gstride, int kk, double* __restrict__ dst, int64_t ldd, EPI... epi) {
  constexpr int LD = 16 * GP + 1;       // staging row of the launch's columns, padded: a column read by 16 rows hits 16 different banks
  constexpr int NS = DIA_TILE / 16;     // strips of a wave
  constexpr int NF = DIA_CHUNK * DIA_TILE / DIA_THREADS;      // slots a thread fetches per chunk
  __shared__ double sv[DIA_CHUNK][DIA_TILE];
  __shared__ double stage[DIA_TILE][LD];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, rr = lane >> 4;
  const int64_t tile0 = (int64_t)blockIdx.x * DIA_TILE;
  int64_t grow[NS];                     // global row of the lane in each strip (a row behind nloc: the last one)
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int64_t lrow = tile0 + wave * 16 + s * 4 + rr;
    grow[s] = row0 + (lrow < nloc ? lrow : nloc - 1);
  }
  double acc[NS][GP];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int g = 0; g < GP; ++g) acc[s][g] = 0.0;
  // the values of a chunk: wave w fetches row `lane` of the tile of diagonals w, w + 4, ... of the chunk
  const int64_t srow = tile0 + lane;
  double pre[NF];
  auto fetch = [&](int d0) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int d = d0 + wave + 4 * f;
      pre[f] = (d < nd && srow < nloc) ? dval[(int64_t)d * ld + srow] : 0.0;
    }
  };
  fetch(0);
  const double* __restrict__ xc = xt + c;
  for (int d0 = 0; d0 < nd; d0 += DIA_CHUNK) {
    __syncthreads();                    // the previous chunk has been read
#pragma unroll
    for (int f = 0; f < NF; ++f) sv[wave + 4 * f][lane] = pre[f];
    __syncthreads();
    if (d0 + DIA_CHUNK < nd) fetch(d0 + DIA_CHUNK);
#pragma unroll
    for (int u0 = 0; u0 < DIA_CHUNK; u0 += DIA_UNROLL) {
      if (d0 + u0 >= nd) break;
      int64_t o[DIA_UNROLL];
#pragma unroll
      for (int u = 0; u < DIA_UNROLL; ++u) o[u] = d0 + u0 + u < nd ? (int64_t)off[d0 + u0 + u] : 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        double v[DIA_UNROLL], x[DIA_UNROLL][GP];
#pragma unroll
        for (int u = 0; u < DIA_UNROLL; ++u) {
          int64_t j = grow[s] + o[u];
          j = j < 0 ? 0 : (j >= n ? n - 1 : j);
#pragma unroll
          for (int g = 0; g < GP; ++g) x[u][g] = xc[(int64_t)g * gstride + j * 16];
          v[u] = sv[u0 + u][wave * 16 + s * 4 + rr];
        }
#pragma unroll
        for (int u = 0; u < DIA_UNROLL; ++u)
          if (d0 + u0 + u < nd) {
#pragma unroll
            for (int g = 0; g < GP; ++g) acc[s][g] = __builtin_fma(v[u], x[u][g], acc[s][g]);
          }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int g = 0; g < GP; ++g) stage[wave * 16 + s * 4 + rr][16 * g + c] = acc[s][g];
  __syncthreads();
  // column-major store of the staged rows: lane = (column offset cc, row r16), 16 consecutive rows of 4 columns per instruction
  const int r16 = lane & 15, cc = lane >> 4;
  const int64_t lrow = tile0 + wave * 16 + r16;
  if (lrow < nloc) {
    if constexpr (sizeof...(EPI) > 0) {
      for (int cl = cc; cl < kk; cl += 4) dst[(int64_t)cl * ldd + lrow] = dia_epilogue(stage[wave * 16 + r16][cl], lrow, cl, epi...);
    } else {
      for (int cl = cc; cl < kk; cl += 4) dst[(int64_t)cl * ldd + lrow] = stage[wave * 16 + r16][cl];
    }
  }
}

template <class... EPI>
void spmm_dia_launch(hipStream_t st, const int32_t* off, int nd, const double* dval, int64_t ld, int64_t nloc, int64_t row0, int64_t n,
                     const double* xt, int64_t xt_gstride, int groups, int kk, double* dst, int64_t ldd, EPI... epi) {
  if (nloc <= 0 || kk <= 0) return;
  const dim3 grid((unsigned)((nloc + DIA_TILE - 1) / DIA_TILE)), block(DIA_THREADS);
  if (groups == 1)
    hipLaunchKernelGGL((spmm_dia_kernel<1, EPI...>), grid, block, 0, st, off, nd, dval, ld, nloc, row0, n, xt, xt_gstride, kk, dst, ldd, epi...);
  else if (groups == 2)
    hipLaunchKernelGGL((spmm_dia_kernel<2, EPI...>), grid, block, 0, st, off, nd, dval, ld, nloc, row0, n, xt, xt_gstride, kk, dst, ldd, epi...);
  else
    hipLaunchKernelGGL((spmm_dia_kernel<4, EPI...>), grid, block, 0, st, off, nd, dval, ld, nloc, row0, n, xt, xt_gstride, kk, dst, ldd, epi...);
}

template <class RP>
void dia_mark_cols(hipStream_t st, const RP* rp, const void* col, int ci64, int64_t n, int64_t nnz, int base, int lower, uint8_t* marks,
                   unsigned long long* ndiag) {
  const int grid = (int)std::min<int64_t>((nnz + DIA_THREADS - 1) / DIA_THREADS, 4096);
  if (ci64) hipLaunchKernelGGL((dia_mark_kernel<RP, int64_t>), dim3(grid), dim3(DIA_THREADS), 0, st, rp, (const int64_t*)col, n, nnz, base, lower, marks, ndiag);
  else hipLaunchKernelGGL((dia_mark_kernel<RP, int32_t>), dim3(grid), dim3(DIA_THREADS), 0, st, rp, (const int32_t*)col, n, nnz, base, lower, marks, ndiag);
}
}  // namespace

void launch_dia_mark(hipStream_t st, const void* row_ptr, int rp64, const void* col_idx, int ci64, int64_t n, int64_t nnz, int base, int lower,
                     uint8_t* marks, unsigned long long* ndiag) {
  if (nnz <= 0 || n <= 0) return;
  if (rp64) dia_mark_cols(st, (const int64_t*)row_ptr, col_idx, ci64, n, nnz, base, lower, marks, ndiag);
  else dia_mark_cols(st, (const int32_t*)row_ptr, col_idx, ci64, n, nnz, base, lower, marks, ndiag);
}

int64_t dia_leading_dimension(int64_t nloc) { return (std::max<int64_t>(nloc, 1) + 15) / 16 * 16; }

void launch_dia_fill(hipStream_t st, const int64_t* rp, const int32_t* col, const double* val, int64_t nloc, int64_t row0, const int32_t* off,
                     int nd, double* dval, int64_t ld) {
  if (nd <= 0) return;
  hipLaunchKernelGGL(dia_fill_kernel, dim3((unsigned)((ld + DIA_THREADS - 1) / DIA_THREADS)), dim3(DIA_THREADS), 0, st, rp, col, val, nloc, row0, off,
                     nd, dval, ld);
}

void launch_spmm_dia(hipStream_t st, const int32_t* off, int nd, const double* dval, int64_t ld, int64_t nloc, int64_t row0, int64_t n,
                     const double* xt, int64_t xt_gstride, int groups, int kk, double* dst, int64_t ldd) {
  spmm_dia_launch(st, off, nd, dval, ld, nloc, row0, n, xt, xt_gstride, groups, kk, dst, ldd);
}

void launch_spmm_dia_cheb(hipStream_t st, const int32_t* off, int nd, const double* dval, int64_t ld, int64_t nloc, int64_t row0, int64_t n,
                          const double* xt, int64_t xt_gstride, int groups, int kk, double* dst, int64_t ldd, const ChebEpi& epi) {
  spmm_dia_launch<ChebEpi>(st, off, nd, dval, ld, nloc, row0, n, xt, xt_gstride, groups, kk, dst, ldd, epi);
}
