// Host-side launchers of the gfx950 kernels (definitions in k_*.hip).  All pointers are device
// pointers; all launches go to the given stream; nothing here synchronises.
#pragma once
#include "common.h"

// ---- K1: block matvec ---------------------------------------------------------------------------
// Row tile of one workgroup (4 waves x 64 rows).  Panels and A are padded to a multiple of it.
constexpr int MV_ROWS = 256;
// Pack k columns of a column-major panel into the transposed MFMA-B layout Xt[group][row][16]
// (zero padded) for rows [0, nloc_pad) of this rank, written at row offset `row_off`.
void launch_pack_xt(hipStream_t st, const double* src, int64_t ld, int64_t nloc, int64_t nslab, int k,
                    double* xt, int64_t xt_group_stride, int64_t row_off);
// slab[s][col][row] = A[rows, chunk s] * X[chunk s, col]; ngroups = ceil(k/16) in {1,2,4}.
void launch_matvec_dense(hipStream_t st, const double* A, int64_t lda, int64_t nrows_pad, int64_t ncols_pad,
                         const double* xt, int64_t xt_group_stride, int ngroups, double* slab,
                         int nsplit, int jc);
void launch_matvec_free(hipStream_t st, OpParams op, int64_t row0, int64_t nloc, int64_t n,
                        int64_t nrows_pad, int64_t ncols_pad, const double* xt, int64_t xt_group_stride,
                        int ngroups, double* slab, int nsplit, int jc);
// dst[i, c] = sum_s slab[s][c][i] for i < nloc_pad (rows >= nloc are written as 0), c < k.
void launch_slab_reduce(hipStream_t st, const double* slab, int nsplit, int64_t nrows_pad, int ngroups,
                        int64_t nloc, int k, double* dst, int64_t ldd);
// scratch (in doubles) one matvec launch needs
size_t matvec_slab_doubles(int64_t nrows_pad, int ngroups, int nsplit);
void matvec_plan(int64_t nrows_pad, int64_t ncols_pad, int ngroups, int* nsplit, int* jc, int64_t target = 0, int64_t forced_nsplit = 0);

// ---- K2: tall-skinny Gram ------------------------------------------------------------------------
constexpr int GRAM_MIN_ROWS = 256; // ... and at least (small problems: more, shorter workgroups)
// out (p x q, column-major ld = p) = P^T Q over nrows_pad rows (multiple of 16; pad rows are zero).
// scratch must hold gram_scratch_doubles(...) doubles.  Deterministic two-stage reduction.
// counters: GRAM_MAX_COUNTERS zeroed device words - with at most GRAM_FUSE_CHUNKS row chunks the workgroup that finishes an output
// tile last sums its partial tiles itself (no second launch); nullptr: always the two-kernel route.
constexpr int GRAM_FUSE_CHUNKS = 24;
constexpr int GRAM_MAX_COUNTERS = 256;
void launch_gram(hipStream_t st, const double* P, int64_t ldp, int p, const double* Q, int64_t ldq, int q,
                 int64_t nrows_pad, double* scratch, double* out_dev, unsigned* counters = nullptr, int wg_target = 0);
size_t gram_scratch_doubles(int p, int q, int64_t nrows_pad);
void gram_set_fuse_chunks(int n);
// C = P^T [Q0 | Q1 | Q2] (p x nq*qeach): the columns of the right-hand side come from up to three blocks of qeach columns each
// (same leading dimension) - the projection and the Gram blocks of one iteration in ONE launch and one reduction (round 5)
void launch_gram_multi(hipStream_t st, const double* P, int64_t ldp, int p, const double* const* Qs, int nq, int qeach, int64_t ldq,
                       int64_t nrows_pad, double* scratch, double* out_dev, unsigned* counters = nullptr, int wg_target = 0);

// ---- K3/K4/K5: panel x small matrix ---------------------------------------------------------------
// The small matrices are passed as MFMA-B OPERAND IMAGES (pg_image_index): for step s (panel columns 4 s .. 4 s + 3) and column
// tile t (output columns 16 t .. 16 t + 15) the 64 values the lanes of a wave need - lane c + 16 g holds M[4 s + g][16 t + c] -
// are contiguous, so a wave fetches them with ONE coalesced 512-byte load.  (Round 3 read M column-major: 16 lines of the cache
// touched per 8-byte load, QT of them per step - what bound the kernel: 0.63 of 8 TB/s at QT = 1, 0.25 at QT = 4.)  tp = tiles
// per step of the image (a multiple of 4, >= ceil(q / 16)); rows past p and columns past q are zero.
struct PanelGemmArgs {
  const double* P1; int64_t ld1; int p1; const double* M1; int64_t tp1;   // term 1 (required)
  const double* P2; int64_t ld2; int p2; const double* M2; int64_t tp2;   // term 2 (p2 = 0: absent)
  double* out; int64_t ldo; int q;          // out[:, 0:q]
  int64_t nloc, nrows_pad;                  // valid rows / padded rows (multiple of 128)
  // epilogue: 0 = store; 1 = DPR: out = acc / (theta[col] * dB[row] - dA[row]) plus column norms;
  //           2 = store plus column norms
  int epilogue;
  const double* theta; const double* dA; const double* dB;   // dB == nullptr: B diagonal = 1
  int nnorm; double* norm_partial;          // [gridDim.x][nnorm] partial sums of acc^2 (cols < nnorm)
  // norm_out != nullptr: the LAST workgroup of the launch sums the partials into norm_out[0:nnorm] (fixed order; replaces the
  // launch of norm_finish_kernel); counter = a zeroed device word (dav_last_workgroup).  For small grids only (PG_FUSE_BLOCKS): the
  // device-scope fence every workgroup pays for the pattern writes its XCD's L2 back - measured at +0.15 ms on the 1563
  // workgroups of N=200000 (and +0.28 ms per sweep when the row-slab block matvec summed its column chunks this way: removed)
  double* norm_out; unsigned* counter;
  int pin;                                  // 1: the pinned software pipeline of the k loop (k_panel.hip), 0: the compiler's order
  // batch > 1 (round 5): the same product on `batch` panels in ONE launch (blockIdx.z): P1, P2 and out of panel z lie batch_stride
  // doubles behind those of panel z - 1 (the basis panel, its image under A and - generalized - under B are neighbours in the
  // engine's arena); same small matrices.  Epilogue 0 only.
  int batch; int64_t batch_stride;
};
// doubles of the operand image of a p x q matrix, its tiles per step, and the index of M[i][j] in it
static inline int64_t pg_image_tiles(int q) { return ((int64_t)(q > 0 ? q : 1) + 63) / 64 * 4; }
static inline int64_t pg_image_doubles(int p, int q) { return ((int64_t)(p > 0 ? p : 1) + 3) / 4 * pg_image_tiles(q) * 64; }
static inline int64_t pg_image_index(int i, int j, int64_t tp) { return (((int64_t)(i >> 2) * tp + (j >> 4)) << 6) + (j & 15) + 16 * (i & 3); }
constexpr int PG_ROWS = 128;
constexpr int PG_FUSE_BLOCKS = 48;         // row blocks up to which the Ritz kernel finishes its own norms (N <= 6144)
constexpr int PG_INPLACE_COLS = 64;       // q <= this: one workgroup column (grid.y == 1), so OUT may alias P1 (see k_panel.hip)
void launch_panel_gemm(hipStream_t st, const PanelGemmArgs& a);
// out[j] = sqrt(sum_b partial[b][j])
void launch_norm_finish(hipStream_t st, const double* partial, int nblocks, int nnorm, double* out);

// ---- setup / utilities ------------------------------------------------------------------------
void launch_generate_dense(hipStream_t st, double* A, int64_t lda, int64_t nrows_pad, int64_t ncols_pad,
                           int64_t row0, int64_t nloc, int64_t n, uint64_t seed, double sparsity,
                           int use_diag, double diag_val);
void launch_diag_dense(hipStream_t st, const double* A, int64_t lda, int64_t row0, int64_t nloc, double* diag);
void launch_diag_free(hipStream_t st, OpParams op, int64_t row0, int64_t nloc, double* diag);
// dst[i, c] = A[i, idx[c]] (column gather: A * unit vectors)
void launch_gather_columns(hipStream_t st, const double* A, int64_t lda, int64_t nrows_pad,
                           const int64_t* idx_dev, int k, double* dst, int64_t ldd);
// dst[:, c] = e_{idx[c]} restricted to local rows
void launch_unit_columns(hipStream_t st, const int64_t* idx_dev, int k, int64_t row0, int64_t nloc,
                         int64_t nrows_pad, double* dst, int64_t ldd);
void launch_copy_columns(hipStream_t st, const double* src, int64_t lds, double* dst, int64_t ldd,
                         int64_t nrows_pad, int k);
// stream microbenchmark over n doubles (n even): mode 0: a = b, mode 1: a = b + s c
void launch_stream(hipStream_t st, int mode, double* a, const double* b, const double* c, double s, int64_t n);
void launch_harness_rate(hipStream_t st, double* out, int wgs, int iters);
// out[i] = sum over p = 0 .. nparts-1 of part_p[i] in that order; part_p = own for p == self, stage + slot(p) * count otherwise (slot = p, minus one behind self)
void launch_compare_blocks(hipStream_t st, const double* a, const double* b, int64_t ld, int64_t rows, int k, double* out);
void launch_poke(hipStream_t st, double* p, double delta);
void launch_sum_parts(hipStream_t st, const double* own, const double* stage, int nparts, int self, size_t count, double* out);



// ---- ingest (k_ingest.hip): row-major staged rows -> resident slab / tiles ----------------------------
// stage: nrows complete rows, row-major (ld = ldr), global rows grow0...; dst = full slab (lda, rows
// [slab_row0, slab_row0 + slab_rows) kept) or, sym != 0, the lower block triangle of SYM_TB tiles.
void launch_rows_scatter(hipStream_t st, const double* stage, int64_t ldr, int64_t grow0, int64_t nrows, int64_t n,
                         double* dst, int64_t lda, int64_t slab_row0, int64_t slab_rows, int sym, const int64_t* row_off);

// ---- K7 helpers (k_gjd.hip) ------------------------------------------------------------------------
struct LincombArgs {      // out[:, j] = sum_t coef[t*ldc + j] * in[t][:, j]
  const double* in[4]; const double* coef; int ldc; int nterms;
  double* out; int64_t ld; int64_t nrows_pad; int m;
};
void launch_lincomb(hipStream_t st, const LincombArgs& a);
void launch_precond(hipStream_t st, const double* in, double* out, int64_t ld, int64_t nloc, int64_t nrows_pad, int m,
                    const double* theta, const double* dA, const double* dB, const double* active);
struct DotsArgs {         // partial[block][s*m + j] = <a[s][:, j], b[s][:, j]> over the block's rows
  const double* a[4]; const double* b[4]; int npairs; int64_t ld; int64_t nrows_pad; int m; double* partial;
};
int coldots_blocks(int64_t nrows_pad);
void launch_coldots(hipStream_t st, const DotsArgs& a);

// ---- K1s: symmetric-tiled storage (k_matvec_sym.hip, k_matvec_sym9.hip) ------------------------------------
constexpr int SYM_TB = 256;     // tile edge; tiles (I, J<=I) contiguous, column-major, ld = SYM_TB
// row_off (device, one entry per block row): first tile of block row I in this rank's storage, -1 = stored by another rank
void launch_matvec_sym(hipStream_t st, const double* tiles, const int64_t* row_off, const int* items_dev, int nitems, const double* xt, int kcols,
                       double* slabD, double* slabT, int npair, int64_t xt_gstride, int64_t slabD_gstride, int64_t slabT_gstride);
// the same sweep with the entries of the hashed operator generated in registers (no stored matrix)
void launch_matvec_sym_generated(hipStream_t st, OpParams op, int64_t n, const int* items_dev, int nitems, const double* xt, int kcols,
                                 double* slabD, double* slabT, int npair, int64_t xt_gstride, int64_t slabD_gstride,
                                 int64_t slabT_gstride);
// accumulate: the sums are ADDED to dst (panel layout only: the second part of an operator that is swept in two parts).
// chunk_rows = 0: dst = panel columns (ldd), rows >= nloc zeroed.  chunk_rows = nslab (several ranks): dst = this rank's
// partial product in reduce-scatter layout [rank][column][row of the rank's slab], rows < total_rows
void launch_sym_reduce(hipStream_t st, const double* slabD, const double* slabT, const int* row_item_begin_dev, const int64_t* owned,
                       int nb, int64_t nloc, int k, double* dst, int64_t ldd, int64_t chunk_rows, int64_t total_rows, bool accumulate = false);
// super-row schedules (k_matvec_sym9.hip): R = 2 or 4 block rows per workgroup, transposed partials summed on chip
void launch_matvec_sym9(hipStream_t st, int R, bool gen, const void* tiles, bool tiles_f32, const int64_t* row_off, OpParams op, int64_t n,
                        int nb, const int* items_dev, int nitems, const int* zslot_begin_dev, const double* xt, int kcols, double* slabD,
                        double* slabT, int npair, int64_t xt_gstride, int64_t slabD_gstride, int64_t slabT_gstride, bool mfma4 = true);
// the same sweep (stored fp64 tiles) with one wave per SIMD and 16 nbw block columns per workgroup (k_matvec_symw.hip): R = 2 block
// rows per workgroup, or (tall, nbw = 1: the work items of the R = 4 schedule) four; nwg workgroups per work item cover the
// 16-column groups [0, nbw nwg) of the block
// tiles_f32 (nbw = 1, R = 2): `tiles` is the fp32 copy of the stored tiles (mixed-precision inner sweeps)
void launch_matvec_symw(hipStream_t st, int nbw, bool tall, bool tiles_f32, const void* tiles, const int64_t* row_off, int nb, const int* items_dev,
                        int nitems, const int* zslot_begin_dev, const double* xt, int kcols, double* slabD, double* slabT, int nwg,
                        int64_t xt_gstride, int64_t slabD_gstride, int64_t slabT_gstride);
void launch_matvec_symw_generated(hipStream_t st, OpParams op, int64_t n, int nb, const int* items_dev, int nitems, const int* zslot_begin_dev,
                                  const double* xt, int kcols, double* slabD, double* slabT, int nwg, int64_t xt_gstride, int64_t slabD_gstride,
                                  int64_t slabT_gstride);
// fp32 copy of `count` stored tile entries (count a multiple of 4)
void launch_tiles_to_f32(hipStream_t st, const double* src, float* dst, int64_t count);
void launch_sym9_reduce(hipStream_t st, const double* slabD, const double* slabT, const int* row_item_begin_dev,
                        const int* zslot_begin_dev, const int64_t* owned, const int* next_owned, int R, int nb, int64_t nloc, int k, double* dst,
                        int64_t ldd, int64_t chunk_rows, int64_t total_rows, bool accumulate = false);
void launch_generate_sym_tiles(hipStream_t st, double* tiles, const int64_t* row_off_host, int nb, int64_t n, uint64_t seed,
                               double sparsity, int use_diag, double diag_val);
void launch_retile_panel(hipStream_t st, const double* panel, int64_t ldp, int64_t nrows, int ncols, int J, int nb,
                         const int64_t* row_off, double* tiles);
void launch_diag_sym(hipStream_t st, const double* tiles, const int64_t* row_off, int64_t n, int64_t nrows, double* diag);
void launch_gather_columns_sym_rs(hipStream_t st, const double* tiles, const int64_t* row_off, int64_t n, int64_t chunk_rows,
                                  int64_t total_rows, const int64_t* idx_dev, int k, double* dst);
// h0[i + j * k] = what this rank's tiles hold of the operator's entry (idx[i], idx[j]) (0 where another rank stores it)
void launch_entries_sym(hipStream_t st, const double* tiles, const int64_t* row_off, const int64_t* idx_dev, int k, double* h0);
void launch_zero_pad_rows(hipStream_t st, double* dst, int64_t ldd, int64_t nloc, int64_t nrows_pad, int k);
void launch_entries_free(hipStream_t st, OpParams op, const int64_t* idx_dev, int k, double* h0);
void launch_entries_dense(hipStream_t st, const double* A, int64_t lda, const int64_t* idx_dev, int k, double* h0);
void launch_gather_columns_free(hipStream_t st, OpParams op, int64_t row0, int64_t nloc, int64_t nrows_pad, const int64_t* idx_dev, int k,
                                double* dst, int64_t ldd);
void launch_gather_columns_sym(hipStream_t st, const double* tiles, const int64_t* row_off, int64_t n, int64_t nrows_pad,
                               const int64_t* idx_dev, int k, double* dst, int64_t ldd);
// dst[i, c] = i < nloc ? src[c * lds + i] : 0 for i < nrows_pad (the received chunk of a reduce-scatter -> panel columns)
void launch_chunk_to_panel(hipStream_t st, const double* src, int64_t lds, int64_t nloc, int64_t nrows_pad, int k, double* dst, int64_t ldd,
                           bool accumulate = false);

// ---- K1c: CSR block product (k_spmm.hip) ----------------------------------------------------------------------------------------------
// Y[rows of this rank, 0:kk] = A_csr * X.  Work list built on the host (engine_sparse.hip: sparse_build_items), one WAVE per item: a run
// of at most CSR_ROWS consecutive whole rows with at most CSR_CHUNK entries together (slot < 0: written to the panel), or one chunk
// of CSR_CHUNK entries of a longer row (slot >= 0: the partial row goes to part[slot][0:64]; launch_spmm_csr_finish adds a row's
// chunks in chunk order).  Every row's sum depends only on its canonical entries, CSR_CHUNK and the launch's column groups.
constexpr int CSR_ROWS = 16;
constexpr int64_t CSR_CHUNK = 1024;   // fixed for every matrix and rank count (multiple of 4 * unroll): the chunk boundaries of a long row
struct CsrItem { int64_t p0, p1; int32_t row, nrows, slot, pad; };
struct CsrLong { int32_t row, first, count, pad; };   // a row longer than CSR_CHUNK: its partials are slots [first, first + count)
// groups = column groups of 16 read per launch (1, 2 or 4); rows [0, nloc) of dst are written, padding rows are not touched
void launch_spmm_csr(hipStream_t st, const CsrItem* items, int nitems, const int64_t* rp, const int32_t* col, const double* val,
                     const double* xt, int64_t xt_gstride, int groups, int kk, double* part, double* dst, int64_t ldd);
void launch_spmm_csr_finish(hipStream_t st, const CsrLong* longs, int nlong, const double* part, int kk, double* dst, int64_t ldd);
// The step of the Chebyshev correction (k_cheb.hip) applied to every finished row value of the product INSTEAD of storing it: with
// y = (A z)[i, j] the element written is cheb_combine(y, z[i, j], r[i, j], zprev[i, j], ...) - the product is never stored and read back.
// z / r / zprev: panel columns of leading dimension ld, column 0 = column 0 of the launch (zprev == nullptr: z_0 = 0, not read);
// hdr / ab / pi: the coefficients cheb_coef left on the device (CHEB_* below), pi[j] of the launch's column j.  Must not alias dst.
struct ChebEpi { const double *z, *r, *zprev, *hdr, *ab, *pi; int64_t ld; };
void launch_spmm_csr_cheb(hipStream_t st, const CsrItem* items, int nitems, const int64_t* rp, const int32_t* col, const double* val,
                          const double* xt, int64_t xt_gstride, int groups, int kk, double* part, double* dst, int64_t ldd, const ChebEpi& epi);
void launch_spmm_csr_finish_cheb(hipStream_t st, const CsrLong* longs, int nlong, const double* part, int kk, double* dst, int64_t ldd,
                                 const ChebEpi& epi);

// ---- K1d: a CSR operator stored by diagonals (k_dia.hip; DAV_CSR_DIAGONALS) ------------------------------------------------------------
// marks[col - row + n - 1] = 1 for every entry of the caller's validated arrays (lower: and for its mirror image), *ndiag += the diagonal
// entries; marks (2 n - 1 bytes) and *ndiag zeroed by the caller
void launch_dia_mark(hipStream_t st, const void* row_ptr, int rp64, const void* col_idx, int ci64, int64_t n, int64_t nnz, int base, int lower,
                     uint8_t* marks, unsigned long long* ndiag);
int64_t dia_leading_dimension(int64_t nloc);     // nloc rounded up to 16 doubles: every diagonal starts 128-byte aligned
// dval[d][i], d < nd, i < ld, from the canonical local rows rp / col / val: +0.0, or the sum from +0.0 of the entries at (i, row0 + i + off[d])
void launch_dia_fill(hipStream_t st, const int64_t* rp, const int32_t* col, const double* val, int64_t nloc, int64_t row0, const int32_t* off,
                     int nd, double* dval, int64_t ld);
// rows [0, nloc) of dst[:, 0:kk] = A X from the packed operand; groups as for launch_spmm_csr; padding rows are not touched
void launch_spmm_dia(hipStream_t st, const int32_t* off, int nd, const double* dval, int64_t ld, int64_t nloc, int64_t row0, int64_t n,
                     const double* xt, int64_t xt_gstride, int groups, int kk, double* dst, int64_t ldd);
void launch_spmm_dia_cheb(hipStream_t st, const int32_t* off, int nd, const double* dval, int64_t ld, int64_t nloc, int64_t row0, int64_t n,
                          const double* xt, int64_t xt_gstride, int groups, int kk, double* dst, int64_t ldd, const ChebEpi& epi);

// ---- K1c': device build of a CSR operator (k_csr_build.hip; dav_set_operator_csr_dev) -----------------------------------------------
// The caller's global arrays: row_ptr and col_idx of 32 (rp64 / ci64 = 0) or 64 bits, numbered from `base`.  info[4] (set to ~0 first):
// [0] first row where row_ptr decreases, [1] row_ptr[0], [2] row_ptr[n], [3] first row of 2^32 or more entries.
// dispatch over the index widths of the caller's arrays (row_ptr, col_idx: 32 or 64 bits): f(RP{}, CI{})
template <class F> void cb_dispatch(int rp64, int ci64, F&& f) {
  if (rp64) {
    if (ci64) f(int64_t{}, int64_t{});
    else f(int64_t{}, int32_t{});
  } else {
    if (ci64) f(int32_t{}, int64_t{});
    else f(int32_t{}, int32_t{});
  }
}

void launch_csr_build_rows(hipStream_t st, const void* rp, int rp64, int64_t n, unsigned long long* info);
// entries [0, nnz): first_bad = the first entry with a column out of range or (lower) above the diagonal; dcount / dfirst (zero / ~0
// first) = diagonal entries of every row and the first of them; mcount (zero first, lower) = mirrored entries of every local row
void launch_csr_build_check(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int64_t nnz, int base, int lower,
                            int64_t r0, int64_t nloc, unsigned long long* first_bad, int32_t* mcount, uint32_t* dcount,
                            unsigned long long* dfirst);
// out[0] = row of entry p, out[1] = col_idx[p]
void launch_csr_build_locate(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int base, int64_t p, int64_t* out);
// lrp[0..nloc] = int64 offsets of the canonical local rows (own + mcount entries); tile_sums holds csr_build_scan_tiles(nloc) values
void launch_csr_build_offsets(hipStream_t st, const void* rp, int rp64, int64_t r0, int64_t nloc, const int32_t* mcount, int64_t* lrp,
                              int64_t* tile_sums);
int64_t csr_build_scan_tiles(int64_t m);
// x[0..m) -> its inclusive prefix sums, in place (the scan of the offsets above); tile_sums holds csr_build_scan_tiles(m) values
void launch_csr_build_scan(hipStream_t st, int64_t* x, int64_t m, int64_t* tile_sums);
// entries [p_lo, p_hi): own entries of local rows and (lower) mirrored entries to the canonical rows, columns narrowed to int32 without
// the base; fill (zero first) = slots taken per local row; tie (lower: required; full: nullptr) = offset of each entry in its source row
void launch_csr_build_scatter(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, const double* vals, int64_t n, int64_t p_lo,
                              int64_t p_hi, int base, int lower, int64_t r0, int64_t nloc, const int64_t* lrp, int32_t* fill, int32_t* ocol,
                              double* oval, uint32_t* tie);
// the same over the block rows of a BSR matrix: what travels with a block column is the block's source, osrc = input block p << 1 | mirrored
void launch_csr_build_scatter(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int64_t p_lo, int64_t p_hi,
                              int base, int lower, int64_t r0, int64_t nloc, const int64_t* lrp, int32_t* fill, int32_t* ocol, uint64_t* osrc,
                              uint32_t* tie);
// flag[i] = 1 (zero first) where canonical row i is not in key order (column, tie)
void launch_csr_build_flag(hipStream_t st, const int64_t* lrp, int64_t nloc, int64_t lnnz, const int32_t* ocol, const uint32_t* tie,
                           uint8_t* flag);
// flagged rows of at most csr_build_sort_tile() entries sorted in place by key (V: double values, or uint64_t block sources)
template <class V>
void launch_csr_build_sort_rows(hipStream_t st, const int64_t* lrp, int64_t nloc, const uint8_t* flag, int32_t* ocol, V* oval,
                                const uint32_t* tie);
int64_t csr_build_sort_tile();
// one longer row [a, a + m) sorted in place by key; k0 / v0 / k1 / v1: scratch of m keys and values each
template <class V>
void launch_csr_build_sort_long(hipStream_t st, int64_t a, int64_t m, int32_t* ocol, V* oval, const uint32_t* tie, uint64_t* k0, V* v0,
                                uint64_t* k1, V* v1);
// diag[0..n) = the diagonal of the whole matrix (a row's diagonal entries summed in input order from +0.0)
void launch_csr_build_diag(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, const double* vals, int64_t n, int base,
                           const uint32_t* dcount, const unsigned long long* dfirst, double* diag);

// ---- K1c'': device build of a CSR operator from COO triples (k_coo_build.hip; davx_set_operator_coo_dev) ---------------------------------
// The caller's global triples: row and col of 32 (ri64 / ci64 = 0) or 64 bits, numbered from `base`, nnz < 2^32.
// first_bad (~0 first) = the first triple with a row or column out of range or (lower) above the diagonal; lcount[i] (zero first) += the
// entries of local row i, own and (lower) mirrored; dcount[i] (zero first) += the diagonal entries of row i of the whole matrix
void launch_coo_build_check(hipStream_t st, const void* row, int ri64, const void* col, int ci64, int64_t n, int64_t nnz, int base, int lower,
                            int64_t r0, int64_t nloc, unsigned long long* first_bad, unsigned long long* lcount, unsigned long long* dcount);
// out[0] = row_idx[p], out[1] = col_idx[p]
void launch_coo_build_locate(hipStream_t st, const void* row, int ri64, const void* col, int ci64, int64_t p, int64_t* out);
// validated triples to atomic slots of their canonical rows: cursor[i] (the row's offset first) counts the slots taken; column, payload
// (V: the value, or the source p << 1 | mirrored) and tie = p per slot.  The diagonal entries also go to slots of the diagonal pattern
// (dcursor: its offsets first): dtie = p, dpos = p
template <class V>
void launch_coo_build_scatter(hipStream_t st, const void* row, int ri64, const void* col, int ci64, const double* vals, int64_t nnz, int base,
                              int lower, int64_t r0, int64_t nloc, unsigned long long* cursor, int32_t* ocol, V* oval, uint32_t* tie,
                              unsigned long long* dcursor, uint32_t* dtie, uint64_t* dpos);
// every row of 2 .. coo_sort_small_rows() entries sorted in place by key (column, tie), in registers - columns, payloads and ties alike,
// so that a later flag pass finds these rows in key order; other rows are left alone
template <class V>
void launch_coo_sort_small(hipStream_t st, const int64_t* lrp, int64_t nrows, int32_t* ocol, V* oval, uint32_t* tie);
int64_t coo_sort_small_rows();
// launch_dia_mark over triples
void launch_coo_mark(hipStream_t st, const void* row, int ri64, const void* col, int ci64, int64_t n, int64_t nnz, int base, int lower,
                     uint8_t* marks, unsigned long long* ndiag);

// ---- factorized sparse approximate inverse (k_fsai.hip; davp_build_fsai) ------------------------------------------
// rp / col: the canonical rows of a CSR operator whose local rows are the whole matrix (one rank), columns ascending.  A pattern is a CSR
// index pair (offsets from 0, columns ascending, the row's own index last) of at most FSAI_MAX_ROW columns per row.
constexpr int FSAI_MAX_ROW = 64;
// level 1: count[i] = columns of P_1(i) (the distinct columns <= i of row i, and i); *bad (~0 first) = the smallest row with more than
// FSAI_MAX_ROW of them.  The fill pass writes them behind the scanned counts prp.
void launch_fsai_pattern1_count(hipStream_t st, const int64_t* rp, const int32_t* col, int64_t n, int64_t* count, unsigned long long* bad);
void launch_fsai_pattern1_fill(hipStream_t st, const int64_t* rp, const int32_t* col, int64_t n, const int64_t* prp, int32_t* pcol);
// the next level: the union of P_1(j) over the columns j of the previous level's row (qrp / qcol), by a merge over the sorted lists
void launch_fsai_pattern_next_count(hipStream_t st, const int64_t* qrp, const int32_t* qcol, const int64_t* p1rp, const int32_t* p1col, int64_t n,
                                    int64_t* count, unsigned long long* bad);
void launch_fsai_pattern_next_fill(hipStream_t st, const int64_t* qrp, const int32_t* qcol, const int64_t* p1rp, const int32_t* p1col, int64_t n,
                                   const int64_t* prp, int32_t* pcol);
// info[0] = the longest row of the offsets rp[0..n], info[1] / info[2] = 1 where a row of at most 16 / of more entries exists; info is 0 first
void launch_fsai_row_lengths(hipStream_t st, const int64_t* rp, int64_t n, unsigned long long* info);
// the rows of G on the pattern prp / pcol: gval[prp[i] + p] = G(i, J_p) and grow[prp[i] + p] = i; brp = nullptr: B is the identity; *bad
// (~0 first) = the smallest row with a pivot that is not finite or not > 0.  small / large: rows of at most 16 / of more columns exist
void launch_fsai_rows(hipStream_t st, const int64_t* prp, const int32_t* pcol, int64_t n, const int64_t* arp, const int32_t* acol,
                      const double* aval, const int64_t* brp, const int32_t* bcol, const double* bval, double sigma, bool small, bool large,
                      double* gval, int32_t* grow, unsigned long long* bad);

// ---- block factorized sparse approximate inverse (k_bfsai.hip; davq_build_block_fsai) ------------------------------
// The pattern is that of the section above over the nb block rows of a BSR operator of block size b (the four pattern launches serve the
// block index arrays unchanged); a block row of m blocks makes s = m b scalar columns, at most BFSAI_MAX_COLS.
constexpr int BFSAI_MAX_COLS = 64;
// after a count pass: *bad = min(*bad, the smallest block row with count[i] * b > BFSAI_MAX_COLS)
void launch_bfsai_cap(hipStream_t st, const int64_t* count, int64_t nb, int b, unsigned long long* bad);
// info[0] = the longest block row of the offsets rp[0..nb], info[1] / info[2] = 1 where a block row of at most 16 / of more scalar columns
// exists; info is 0 first
void launch_bfsai_row_lengths(hipStream_t st, const int64_t* rp, int64_t nb, int b, unsigned long long* info);
// the block rows of G on the pattern prp / pcol: gval[(prp[I] + q) b^2 + t b + r] = G(I b + t, J_q b + r) and grow[prp[I] + q] = I; brp =
// nullptr: B is the identity; *bad (~0 first) = the smallest block row with a pivot that is not finite or not > 0
void launch_bfsai_rows(hipStream_t st, const int64_t* prp, const int32_t* pcol, int64_t nb, int b, const int64_t* arp, const int32_t* acol,
                       const double* aval, const int64_t* brp, const int32_t* bcol, const double* bval, double sigma, bool small, bool large,
                       double* gval, int32_t* grow, unsigned long long* bad);
// the block rows of G^T: count[c] += 1 per block of block column c (count is 0 first; launch_csr_build_scan makes the offsets trp of it),
// then every block takes a slot of its block column (cursor is 0 first; slot holds nnzb values) and is copied there untouched
void launch_bfsai_transpose_count(hipStream_t st, const int32_t* pcol, int64_t nnzb, int64_t* count);
void launch_bfsai_transpose_fill(hipStream_t st, const int32_t* pcol, const int32_t* grow, const double* gval, int64_t nnzb, int b,
                                 const int64_t* trp, int64_t* cursor, int64_t* slot, int32_t* tcol, double* tval);

// ---- K1d': device build of a BSR operator (k_bsr_build.hip; dav_set_operator_bsr_dev) -----------------------------------------------
// The index level is the CSR build above over the n / b block rows with the block source as payload.  Then the values move once:
// val[q b^2 + k b + m] = entry (tr ? k : m, tr ? m : k) of input block p, for canonical block q with src[q] = p << 1 | tr; rowmaj: the
// caller's blocks are row-major.  vals holds the caller's nnzb blocks, every p < nnzb.
void launch_bsr_build_gather(hipStream_t st, int bs, const uint64_t* src, int64_t lnnzb, const double* vals, int rowmaj, double* val);
// diag[0..n) = the diagonal of the whole matrix: per block row the diagonal entries of its diagonal blocks, summed in input order from
// +0.0 (dcount / dfirst of the check pass over the block rows; entry (m, m) sits at m b + m in either layout)
void launch_bsr_build_diag(hipStream_t st, int bs, const void* rp, int rp64, const void* col, int ci64, const double* vals, int64_t nb,
                           int base, const uint32_t* dcount, const unsigned long long* dfirst, double* diag);
// The (re, im) value source of a complex Hermitian CSR matrix (davh_set_operator_csr(_dev), b = 2): pairs[2 p], pairs[2 p + 1] = (a, b) of
// entry p stand for the block [[a, -b], [b, a]], 16-byte aligned.  val[4 q ..] = tr ? {a, -b, b, a} : {a, b, -b, a} (column-major).
void launch_bsr_build_gather_pairs(hipStream_t st, const uint64_t* src, int64_t lnnzb, const double* pairs, double* val);
// diag[2 I] = diag[2 I + 1] = +0.0 + the real parts of the diagonal entries of row I in input order, I < nb; *bad (~0 first) = the smallest
// position of a diagonal entry whose imaginary part is not +-0.0.  The second form reads the kept diagonal sources (the refresh).
void launch_bsr_build_diag_pairs(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, const double* pairs, int64_t nb, int base,
                                 const uint32_t* dcount, const unsigned long long* dfirst, double* diag, unsigned long long* bad);
void launch_bsr_refresh_diag_pairs(hipStream_t st, const int64_t* doff, const int64_t* dpos, const double* pairs, int64_t nb, double* diag,
                                   unsigned long long* bad);

// ---- K1e: new values on the kept pattern of a sparse operator (k_sparse_refresh.hip; dav_update_operator_values) --------------------
// The value map src[q] = p << 1 | mirrored of every canonical local entry (block) q, p the position in the caller's vals, and the
// diagonal sources of the whole matrix: dpos[doff[I] .. doff[I + 1]) = the positions of the diagonal entries (blocks) of row (block
// row) I in input order.
// CSR: val[q] = vals[src[q] >> 1] over the lnnz local entries (BSR: launch_bsr_build_gather); sparse_refresh_tile() entries per workgroup
void launch_sparse_refresh_csr(hipStream_t st, const uint64_t* src, int64_t lnnz, const double* vals, double* val);
int64_t sparse_refresh_tile();
// diag[i] = +0.0 + entry (m, m), m = i mod bs, of the diagonal blocks of block row i / bs in input order, i < n (the whole matrix);
// entry (m, m) of block p sits at p bs^2 + m bs + m in either block layout.  bs = 1: a CSR matrix
void launch_sparse_refresh_diag(hipStream_t st, int bs, const int64_t* doff, const int64_t* dpos, const double* vals, int64_t n, double* diag);
// the device set entries, after the check pass (dcount / dfirst of launch_csr_build_check over the n rows or block rows):
// doff[0] = 0, doff[i + 1] = dcount[i] (then launch_csr_build_scan over doff + 1), and dpos behind the scanned offsets
void launch_sparse_build_diag_counts(hipStream_t st, const uint32_t* dcount, int64_t n, int64_t* doff);
void launch_sparse_build_diag_sources(hipStream_t st, const void* rp, int rp64, const void* col, int ci64, int64_t n, int base,
                                      const uint32_t* dcount, const unsigned long long* dfirst, const int64_t* doff, int64_t* dpos);

// ---- K1d: BSR block product on the matrix cores (k_bsrmm.hip) ------------------------------------------------------------------------
// Y[rows of this rank, 0:kk] = A_bsr * X, uniform block size 1 <= b <= 16, blocks column-major on the device.  Work list built on the
// host (engine_sparse.hip: sparse_build_items) in the CSR item types over LOCAL block rows: a run of whole block rows of at most BSR_ROWS
// matrix rows and BSR_CHUNK blocks together (slot < 0), or one chunk of BSR_CHUNK blocks of a longer block row (slot >= 0: the partial
// block row goes to part[slot][16][64]; launch_spmm_bsr_finish adds a block row's chunks in chunk order).  The rows written are the
// local rows [0, nloc) of the block rows; the first row of local block row 0 is local row grow0 (<= 0).
constexpr int BSR_ROWS = 16;
constexpr int64_t BSR_CHUNK = 128;    // blocks; fixed for every matrix and rank count: the chunk boundaries of a long block row
void launch_spmm_bsr(hipStream_t st, const CsrItem* items, int nitems, int bs, const int64_t* rp, const int32_t* col, const double* val,
                     const double* xt, int64_t xt_gstride, int groups, int kk, double* part, double* dst, int64_t ldd, int64_t grow0,
                     int64_t nloc);
void launch_spmm_bsr_finish(hipStream_t st, const CsrLong* longs, int nlong, const double* part, int bs, int kk, double* dst, int64_t ldd,
                            int64_t grow0, int64_t nloc);

// ---- device-side Rayleigh-Ritz (k_smalleig.hip): all eigenpairs of H y = theta y / H y = theta S y, order m <= 128 ------
// info[0] of the kernel: sweeps used (0 .. EIG_MAX_SWEEPS - 1), -j for a non-positive Cholesky pivot j (1 .. 128), or one of
constexpr int EIG_MAX_SWEEPS = 30;
constexpr int EIG_INFO_NOT_FINITE = -1000;       // a NaN / Inf entry in H, S or the reduced matrix
constexpr int EIG_INFO_NOT_CONVERGED = -2000;    // a rotation still pending after EIG_MAX_SWEEPS sweeps
size_t small_eig_work_doubles(int m);
bool launch_small_eig(hipStream_t st, const double* H, int64_t ldh, const double* S, int64_t lds, int m, bool gev, double* theta,
                      double* Y, int64_t ldy, double* work, double* info);
void launch_rr_scatter(hipStream_t st, const double* blk, int mt, int k, int c0, double* Hd, int64_t ld);
void launch_rr_pack(hipStream_t st, const double* Y, int64_t ld, const double* theta, int m, int q, int ldm, int qpad, double* Ypk,
                    double* Y2pk, double* theta_pk, const double* info, double* result_tail);
// ---- k_guess.hip: ingest of an initial guess -----------------------------------------------------------------------------------------------
// dst[0:nrows, c] = src[0:nrows, c] (bit for bit), dst[nrows:nrows + npad, c] = +0.0 for c < ncols; flags (guess_flag_words(ncols) words,
// zeroed by the caller before the first launch of a guess): word 0 |= 1 when an entry is Inf or NaN, word 1 + c / 64 |= 1 << c % 64 when
// column c holds a non-zero.  16-byte lanes when guess_ingest_wide says both sides allow them, 8-byte lanes otherwise.
int guess_flag_words(int ncols);
bool guess_ingest_wide(const double* src, int64_t ldx, const double* dst, int64_t ldd);
void launch_guess_ingest(hipStream_t st, const double* src, int64_t ldx, int64_t nrows, int ncols, int64_t npad, double* dst, int64_t ldd,
                         unsigned long long* flags);

// ---- k_bdpr.hip: block-diagonal preconditioned correction of a BSR operator (DAV_METHOD_BDPR) --------------------------------------------
// out[I b^2 + k b + m] = entry (m, k) of the diagonal block of local block row I < nbl (global block row ib0 + I) of the canonical store
// rp / col / val: the row's blocks with that block column added in stored order from +0.0; no such block: zeros
void launch_bdpr_diag_blocks(hipStream_t st, int bs, const int64_t* rp, const int32_t* col, const double* val, int64_t nbl, int64_t ib0, double* out);
// T[I b .. (I + 1) b, j] = (theta[j] B_II - A_II)^-1 R[I b .. (I + 1) b, j] for I < nbl, j < ncols (nbl * bs = nloc): Gaussian elimination with
// partial pivoting (largest magnitude, ties to the lowest row), an exactly zero pivot gives +0.0 for that block and column.  dA / dB: the
// diagonal blocks as launch_bdpr_diag_blocks leaves them, dB == nullptr: B_II = I.  Rows [nloc, nrows_pad) of the ncols columns of T are
// written as +0.0.  1 <= bs <= 16
void launch_bdpr_solve(hipStream_t st, int bs, const double* dA, const double* dB, const double* theta, const double* R, int64_t ldr, double* T,
                       int64_t ldt, int ncols, int64_t nbl, int64_t nloc, int64_t nrows_pad);

// ---- k_cheb.hip: Chebyshev-filtered correction of a sparse operator (DAV_METHOD_CHEB; engine_cheb.hip) ---------------------------------
constexpr int CHEB_MAX_DEGREE = 64;
constexpr int CHEB_DEFAULT_DEGREE = 10;
constexpr int CHEB_BOUND_PARTIALS = 1024;      // workgroups of the row-sum kernel at the most: one partial maximum each
// Coefficients of one correction, on the device: coef[CHEB_VALID] = 1.0 when the interval is usable (0.0: the block is +0.0),
// coef[CHEB_C] = c, coef[CHEB_AB + 2 k] / [.. + 1] = alpha_k / beta_k of the step that makes z_{k+1} from z_k (k = 0: alpha_0 = s_1 / e of
// z_1 = alpha_0 r, beta_0 = 0), then pi_k of column j at coef[CHEB_PI + k * pstride + j].
constexpr int CHEB_VALID = 0, CHEB_C = 1, CHEB_AB = 2, CHEB_PI = CHEB_AB + 2 * CHEB_MAX_DEGREE + 6;   // 136: the rows of pi start 16-byte aligned
inline size_t cheb_coef_doubles(int ncols) { return (size_t)CHEB_PI + (size_t)CHEB_MAX_DEGREE * (size_t)((ncols + 63) / 64 * 64); }
// The one statement of a step's arithmetic, shared by cheb_step and the epilogue of the CSR product (their bits must agree):
//   t = fma(-c, z, y);  t = fma(pi, r, t);  u = alpha * t;  result = fma(-beta, zprev, u)   (no zprev: u);  not valid: +0.0
__device__ __forceinline__ double cheb_combine(double y, double z, double r, double zprev, bool has_prev, double c, double pi, double alpha,
                                               double beta, bool valid) {
#pragma clang fp contract(off)
  double t = __builtin_fma(-c, z, y);
  t = __builtin_fma(pi, r, t);
  const double u = alpha * t;
  const double o = has_prev ? __builtin_fma(-beta, zprev, u) : u;
  return valid ? o : 0.0;
}
// slots[rank] = max over the stored rows of sum_j |a_ij| (rows of the nbl local block rows of block size bs, bs = 1: CSR rows; a row's
// entries added in stored order from +0.0; NaN propagates), slots[p] = +0.0 for the other p < nranks; partial: CHEB_BOUND_PARTIALS doubles
void launch_cheb_row_bound(hipStream_t st, int bs, const int64_t* rp, const double* val, int64_t nbl, double* partial, double* slots, int rank,
                           int nranks);
// the same bound of an operator stored by diagonals: the row sums of |dval[d][i]|, d ascending from +0.0, over the nloc local rows (fill
// slots add +0.0: without duplicates the bits of the CSR bound of the same matrix)
void launch_dia_row_bound(hipStream_t st, const double* dval, int64_t ld, int nd, int64_t nloc, double* partial, double* slots, int rank, int nranks);
// the interval and the coefficients of a correction of `degree` from theta[0 .. ncorr) and max(slots[0 .. nranks)): one lane per column
void launch_cheb_coef(hipStream_t st, const double* theta, int ncorr, int lowest, int degree, const double* slots, int nranks, double* coef,
                      int pstride);
// out[:, j] = cheb_combine(az[:, j], z[:, j], r[:, j], zprev[:, j]) with step k's coefficients for j < ncols, rows [0, nloc); rows [nloc,
// nrows_pad) are written as +0.0.  k = 0: out = alpha_0 r (az, z, zprev not read).  zprev == nullptr: not read.  out may be zprev.
void launch_cheb_step(hipStream_t st, int k, const double* coef, int pstride, const double* az, const double* z, const double* r, const double* zprev,
                      double* out, int64_t ld, int ncols, int64_t nloc, int64_t nrows_pad);

// ---- k_lanczos.hip: the vector work of the Lanczos bound (DAV_METHOD_LCHEB; engine_cheb.hip) ---------------------------------------------
constexpr int LANCZOS_STEPS = 12;
// Each launch leaves the sum of its dot product over this rank's rows in slots[rank] and +0.0 in slots[p] of the other p < nranks; partial:
// lanczos_partials(nrows_pad) doubles, one per workgroup.  Vectors: nrows_pad doubles (even), rows [nloc, nrows_pad) are written as +0.0.
int lanczos_partials(int64_t nrows_pad);
// u[i] = (splitmix64(row0 + i + 1) >> 11) * 2^-52 - 1;  <u, u>
void launch_lanczos_start(hipStream_t st, double* u, int64_t row0, int64_t nloc, int64_t nrows_pad, double* partial, double* slots, int rank,
                          int nranks);
// v = u / nrm over u,  w = au / nrm - beta * vprev over au (vprev == nullptr: not read);  <v, w>
void launch_lanczos_first(hipStream_t st, double* u, double* au, const double* vprev, double nrm, double beta, int64_t nloc, int64_t nrows_pad,
                          double* partial, double* slots, int rank, int nranks);
// w -= alpha * v;  <w, w>
void launch_lanczos_second(hipStream_t st, double* w, const double* v, double alpha, int64_t nloc, int64_t nrows_pad, double* partial,
                           double* slots, int rank, int nranks);
