// K1d: block product of a BSR operator, Y[rows of this rank, 0:kk] = A_bsr * X (dav_set_operator_bsr), on the matrix cores.
//
// X arrives in the packed operand of the row-slab path (launch_pack_xt, all-gathered over the ranks): xt[g][j * 16 + c] = X[j, 16 g + c],
// which is the B operand of both f64 MFMA shapes as it stands - lane l reads row (block column J) * b + 4 s + (l >> 4), column 16 g +
// (l & 15): four consecutive rows of a 16-column group are four contiguous 128-byte segments.  A block is stored column-major on the
// device (val[blk * b * b + k * b + m] = A_blk[m][k], whatever the caller's layout), so one K-step of the A operand is 4 b (for b = 16:
// 64) consecutive doubles.  Block sizes are padded to multiples of 4 in registers, never in memory: rows / columns k >= b load zeros.
//
// Lane mapping (common.h and k_matvec_sym9.hip give the operand layouts):
//   b <= 8  (M4): v_mfma_f64_4x4x4_4b_f64; the four 4x4 blocks of one instruction are the four 4-column quarters of a 16-column group,
//                 A is replicated over them (lane l holds A[4 q + (l & 3)][4 s + (l >> 4)]).  NQ = ceil(b / 4) row quarters q x NQ
//                 K-steps s per block and group: 1 instruction at b <= 4, 4 at b = 8.  D: one double per row quarter, row 4 q + (l >> 4).
//   b >= 9  (M16): v_mfma_f64_16x16x4_f64, lane l holds A[l & 15][4 s + (l >> 4)]; ceil(b / 4) K-steps per block and group, 4 at b = 16.
//                 D: four doubles, row (l >> 4) + 4 r.
// Either way accumulator t of group g in lane l is Y[row (l >> 4) + 4 t of the block row, column 16 g + (l & 15)].
//
// One wave per work item (kernels.h: BSR_ROWS, BSR_CHUNK): a run of whole block rows of at most BSR_ROWS matrix rows and BSR_CHUNK
// blocks together, or one chunk of BSR_CHUNK blocks of a longer block row.  A block row sums its blocks in canonical order and the
// K-steps of a block in order; the chunks of a long block row are added in chunk order by the finishing pass.  No atomics: the bits of
// a row depend on its canonical blocks, b and BSR_CHUNK only - not on the rank count, the column groups, the work list or the launch.
// A rank computes every block row that touches its slab and writes only its own rows (for b outside {1, 2, 4, 8, 16} a block row may
// straddle two slabs).
//
// Results of whole block rows are staged in LDS ([row][column], at most 16 rows of 16 GP columns per wave) and stored column by column:
// up to 16 consecutive rows of a panel column per quarter-wave.  Partial block rows of chunks go to part[slot][16 rows][64 columns].
#include "kernels.h"

namespace {
__device__ __forceinline__ double mfma4x4_f64(double a, double b, double c) { return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0); }

// blocks whose index and operand loads are issued before their MFMAs: about 16 B-operand doubles per lane in flight, 1..4 blocks
template <int NS, int GP> constexpr int bsr_unroll() {
  return 16 / (NS * GP) < 1 ? 1 : (16 / (NS * GP) > 4 ? 4 : 16 / (NS * GP));
}
}  // namespace

// NS = ceil(b / 4) K-steps; M16: the 16x16x4 shape (b >= 9), else the 4x4x4 one with NS row quarters.  Item rows are LOCAL block rows
// (indices into rp); the first row of local block row lr is local output row grow0 + lr * b (grow0 <= 0: the first block row may begin
// on the previous rank).
template <int NS, bool M16, int GP>
__global__ __launch_bounds__(256) void spmm_bsr_kernel(const CsrItem* __restrict__ items, int nitems, int bs, const int64_t* __restrict__ rp,
                                                       const int32_t* __restrict__ col, const double* __restrict__ val,
                                                       const double* __restrict__ xt, int64_t gstride, int kk, double* __restrict__ part,
                                                       double* __restrict__ dst, int64_t ldd, int64_t grow0, int64_t nloc) {
  constexpr int NT = M16 ? 4 : NS;        // accumulator doubles per group
  constexpr int NA = M16 ? NS : NS * NS;  // A-operand doubles per block
  constexpr int U = bsr_unroll<NS, GP>();
  constexpr int LD = 16 * GP + 1;         // staging row of the launch's columns, padded: a column read by 16 rows hits 16 different banks
  __shared__ double stage[4][BSR_ROWS][LD];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, h = lane >> 4;
  const int it = blockIdx.x * 4 + wave;
  int64_t p0 = 0, p1 = 0;
  int brow = 0, nbrows = 0, slot = -1;
  if (it < nitems) {
    const CsrItem item = items[it];
    p0 = item.p0; p1 = item.p1; brow = item.row; nbrows = item.nrows; slot = item.slot;
  }
  const int64_t bb = (int64_t)bs * bs;
  // this lane's place in a block: offsets of its A-operand doubles (column-major block) and which K-steps of B lie inside the block
  int aoff[NA];
  bool aok[NA];
#pragma unroll
  for (int q = 0; q < NA; ++q) {
    const int s = q % NS, m = M16 ? c : 4 * (q / NS) + (lane & 3), k = 4 * s + h;
    aok[q] = m < bs && k < bs;
    aoff[q] = aok[q] ? k * bs + m : 0;
  }
  bool bok[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) bok[s] = 4 * s + h < bs;
  const double* __restrict__ xl = xt + (h * 16 + c);
  for (int r = 0; r < nbrows; ++r) {
    const int64_t a = slot >= 0 ? p0 : rp[brow + r];
    const int64_t e = slot >= 0 ? p1 : rp[brow + r + 1];
    double acc[GP][NT];
#pragma unroll
    for (int g = 0; g < GP; ++g)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[g][t] = 0.0;
    for (int64_t p = a; p < e; p += U) {
      int64_t xo[U];
      double av[U][NA], xv[U][GP][NS];
#pragma unroll
      for (int u = 0; u < U; ++u) xo[u] = p + u < e ? (int64_t)col[p + u] * bs * 16 : 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double* __restrict__ vb = val + (p + u < e ? (p + u) * bb : 0);
#pragma unroll
        for (int q = 0; q < NA; ++q) av[u][q] = (p + u < e && aok[q]) ? vb[aoff[q]] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int g = 0; g < GP; ++g)
#pragma unroll
          for (int s = 0; s < NS; ++s) xv[u][g][s] = (p + u < e && bok[s]) ? xl[(int64_t)g * gstride + xo[u] + 64 * s] : 0.0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (p + u >= e) break;
#pragma unroll
        for (int g = 0; g < GP; ++g) {
          if constexpr (M16) {
            f64x4 d = {acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
#pragma unroll
            for (int s = 0; s < NS; ++s) d = mfma_f64(av[u][s], xv[u][g][s], d);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[g][t] = d[t];
          } else {
#pragma unroll
            for (int q = 0; q < NS; ++q)
#pragma unroll
              for (int s = 0; s < NS; ++s) acc[g][q] = mfma4x4_f64(av[u][q * NS + s], xv[u][g][s], acc[g][q]);
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < GP; ++g)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int m = h + 4 * t;
        if (m < bs) {
          if (slot >= 0) part[(int64_t)slot * 1024 + m * 64 + 16 * g + c] = acc[g][t];
          else stage[wave][r * bs + m][16 * g + c] = acc[g][t];
        }
      }
  }
  __syncthreads();
  if (slot >= 0) return;
  // column-major store of the staged rows that lie in this rank's slab: lane = (column offset cc, row rr), 16 rows of 4 columns per step
  const int rr = lane & 15, cc = lane >> 4;
  const int64_t lrow = grow0 + (int64_t)brow * bs + rr;
  if (rr < nbrows * bs && lrow >= 0 && lrow < nloc)
    for (int cl = cc; cl < kk; cl += 4) dst[(int64_t)cl * ldd + lrow] = stage[wave][rr][cl];
}

// one wave per long block row: lane = column; for each of its b rows in this rank's slab the chunk partials added in chunk order
__global__ __launch_bounds__(64) void spmm_bsr_finish_kernel(const CsrLong* __restrict__ longs, const double* __restrict__ part, int bs,
                                                             int kk, double* __restrict__ dst, int64_t ldd, int64_t grow0, int64_t nloc) {
  const CsrLong L = longs[blockIdx.x];
  const int lane = threadIdx.x;
  for (int m = 0; m < bs; ++m) {
    const int64_t lrow = grow0 + (int64_t)L.row * bs + m;
    if (lrow < 0 || lrow >= nloc) continue;
    const double* __restrict__ pp = part + (int64_t)L.first * 1024 + m * 64 + lane;
    double sum = pp[0];
    for (int q = 1; q < L.count; ++q) sum += pp[(int64_t)q * 1024];
    if (lane < kk) dst[(int64_t)lane * ldd + lrow] = sum;
  }
}

namespace {
template <int NS, bool M16>
void launch_bsr_ns(hipStream_t st, const CsrItem* items, int nitems, int bs, const int64_t* rp, const int32_t* col, const double* val,
                   const double* xt, int64_t gstride, int groups, int kk, double* part, double* dst, int64_t ldd, int64_t grow0, int64_t nloc) {
  const dim3 grid((unsigned)((nitems + 3) / 4)), block(256);
  if (groups == 1)
    hipLaunchKernelGGL((spmm_bsr_kernel<NS, M16, 1>), grid, block, 0, st, items, nitems, bs, rp, col, val, xt, gstride, kk, part, dst, ldd, grow0, nloc);
  else if (groups == 2)
    hipLaunchKernelGGL((spmm_bsr_kernel<NS, M16, 2>), grid, block, 0, st, items, nitems, bs, rp, col, val, xt, gstride, kk, part, dst, ldd, grow0, nloc);
  else
    hipLaunchKernelGGL((spmm_bsr_kernel<NS, M16, 4>), grid, block, 0, st, items, nitems, bs, rp, col, val, xt, gstride, kk, part, dst, ldd, grow0, nloc);
}
}  // namespace

void launch_spmm_bsr(hipStream_t st, const CsrItem* items, int nitems, int bs, const int64_t* rp, const int32_t* col, const double* val,
                     const double* xt, int64_t xt_gstride, int groups, int kk, double* part, double* dst, int64_t ldd, int64_t grow0,
                     int64_t nloc) {
  if (nitems <= 0 || kk <= 0 || bs < 1 || bs > 16) return;
  switch ((bs + 3) / 4) {
    case 1: launch_bsr_ns<1, false>(st, items, nitems, bs, rp, col, val, xt, xt_gstride, groups, kk, part, dst, ldd, grow0, nloc); break;
    case 2: launch_bsr_ns<2, false>(st, items, nitems, bs, rp, col, val, xt, xt_gstride, groups, kk, part, dst, ldd, grow0, nloc); break;
    case 3: launch_bsr_ns<3, true>(st, items, nitems, bs, rp, col, val, xt, xt_gstride, groups, kk, part, dst, ldd, grow0, nloc); break;
    default: launch_bsr_ns<4, true>(st, items, nitems, bs, rp, col, val, xt, xt_gstride, groups, kk, part, dst, ldd, grow0, nloc); break;
  }
}

void launch_spmm_bsr_finish(hipStream_t st, const CsrLong* longs, int nlong, const double* part, int bs, int kk, double* dst, int64_t ldd,
                            int64_t grow0, int64_t nloc) {
  if (nlong <= 0 || kk <= 0) return;
  hipLaunchKernelGGL(spmm_bsr_finish_kernel, dim3((unsigned)nlong), dim3(64), 0, st, longs, part, bs, kk, dst, ldd, grow0, nloc);
}
