// Engine, the built block preconditioner: davq_build_block_fsai puts the block factorized sparse approximate inverse M = G^T G of
// A - sigma B, A a BSR operator, into slot DAV_OP_M (include/davidson_hip_bprecond.h has the definition; kernels in k_bfsai.hip and the
// pattern launches of k_fsai.hip).
// Steps: the scalar checks and the kinds of A and B; the pattern of tril(A)^level over the block index arrays, level by level - a count
// pass, the cap m b <= 64 with the first block row above it refused, the engine's scan (k_csr_build.hip), a fill pass; the block rows of G
// (one dense SPD factorisation of order m b each) with the first failed pivot refused; the slots of G^T; then the two stores, both through
// the device BSR build (dav_set_operator_bsr_dev) on slot M: G from its row-major blocks, G^T from the same blocks declared column-major
// and listed by block column - no block is transposed by hand, both stores are canonical ones with their work lists, and the long block
// rows of G^T get their fixed chunks.  Everything before the two stores lives in scratch: a refusal allocates nothing for the operator.
#include "engine_internal.h"
#include "davidson_hip_bprecond.h"

namespace {
const char* const NAME = "davq_build_block_fsai";

// scratch of a build: released on every way out, after the stream has finished with it
struct Scratch {
  hipStream_t st;
  std::vector<void*> held;
  bool oom = false;
  explicit Scratch(hipStream_t s) : st(s) {}
  Scratch(const Scratch&) = delete;
  ~Scratch() { (void)hipStreamSynchronize(st); for (void* p : held) pool_free(p); }
  template <class T> void take(T** p, size_t count) {
    *p = nullptr;
    if (oom) return;
    if (pool_malloc(p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; oom = true; return; }
    held.push_back((void*)*p);
  }
};

int readback(hipStream_t st, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// a refused build leaves slot M unset (whatever it held) and the engine usable
int refuse(E* e, const std::string& msg) {
  CHK(operator_goes(e, DAV_OP_M, true));
  return fail(std::string(NAME) + ": " + msg);
}

// a HIP failure on the way (fail() has recorded it): slot M is left unset as after a refusal, the recorded message stays
int unset(E* e, int rc) {
  const std::string msg = dav_last_error();
  (void)operator_goes(e, DAV_OP_M, true);
  fail(msg);
  return rc;
}

// hlen[0] = the longest block row of the device offsets rp[0..nb], hlen[1] / hlen[2] = block rows of at most 16 / of more scalar columns exist
int row_lengths(hipStream_t st, const int64_t* rp, int64_t nb, int b, unsigned long long* info, unsigned long long* hlen) {
  HIPCHK(hipMemsetAsync(info, 0, sizeof(unsigned long long) * 3, st));
  launch_bfsai_row_lengths(st, rp, nb, b, info);
  return readback(st, hlen, info, sizeof(unsigned long long) * 3);
}

struct Pattern { int64_t* rp = nullptr; int32_t* col = nullptr; int64_t nnz = 0; };

// One level of the block pattern: the counts behind a leading 0, the refusal of the first block row above the cap, the scan and the fill.
// prev == nullptr: level 1, from the canonical block rows of A; else the next level from *prev and the first level *p1.  why: the refusal.
int pattern_level(E* e, Scratch& sc, const SparseStore& A, int64_t nb, int b, int level, const Pattern* prev, const Pattern* p1,
                  unsigned long long* bad, int64_t* tile_sums, Pattern* out, std::string* why) {
  hipStream_t st = e->stream;
  sc.take(&out->rp, (size_t)nb + 1);
  if (sc.oom) { *why = "device memory for the pattern offsets could not be allocated"; return 1; }
  HIPCHK(hipMemsetAsync(out->rp, 0, sizeof(int64_t), st));
  HIPCHK(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), st));
  if (!prev) launch_fsai_pattern1_count(st, A.rp, A.col, nb, out->rp + 1, bad);
  else launch_fsai_pattern_next_count(st, prev->rp, prev->col, p1->rp, p1->col, nb, out->rp + 1, bad);
  launch_bfsai_cap(st, out->rp + 1, nb, b, bad);          // m b <= 64: m <= 64 follows, the count pass's own minimum is covered
  unsigned long long first_bad = 0;
  CHK(readback(st, &first_bad, bad, sizeof(first_bad)));
  if (first_bad != ~0ull) {
    int64_t len = 0;
    CHK(readback(st, &len, out->rp + 1 + (int64_t)first_bad, sizeof(len)));
    *why = "the pattern of block row " + std::to_string((int64_t)first_bad) + " holds " + std::to_string(len) + " blocks of size " +
           std::to_string(b) + " at level " + std::to_string(level) + ", " + std::to_string(len * b) + " scalar columns: a block row of G holds at most " +
           std::to_string(BFSAI_MAX_COLS) + " (the pattern is never cut)";
    return 1;
  }
  launch_csr_build_scan(st, out->rp + 1, nb, tile_sums);
  CHK(readback(st, &out->nnz, out->rp + nb, sizeof(int64_t)));
  sc.take(&out->col, (size_t)out->nnz);
  if (sc.oom) { *why = "device memory for the pattern of " + std::to_string(out->nnz) + " blocks could not be allocated"; return 1; }
  if (!prev) launch_fsai_pattern1_fill(st, A.rp, A.col, nb, out->rp, out->col);
  else launch_fsai_pattern_next_fill(st, prev->rp, prev->col, p1->rp, p1->col, nb, out->rp, out->col);
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" int davq_build_block_fsai(dav_handle_t e, double sigma, int level) {
  if (!e) return fail(std::string(NAME) + ": null engine");
  CHK(bind(e));
  // ---- the scalar arguments and the operators, before anything is allocated
  if (level < 1 || level > 3) return refuse(e, "level = " + std::to_string(level) + " must lie in 1..3");
  if (!std::isfinite(sigma)) return refuse(e, "sigma is not finite");
  if (e->nranks > 1)
    return refuse(e, "the engine has " + std::to_string(e->nranks) + " ranks: a rank stores only its rows of A and a row of G needs other rows");
  const OpDesc& A = e->op[DAV_OP_A];
  const OpDesc& B = e->op[DAV_OP_B];
  if (A.kind != DAV_KIND_BSR)
    return refuse(e, std::string("operator A is ") + kind_words(A.kind) + ": the build reads the canonical block rows of a BSR operator");
  const int b = A.sp.b;
  const bool b_identity = B.kind == DAV_KIND_NONE || B.kind == DAV_KIND_IDENTITY;
  if (!b_identity && B.kind != DAV_KIND_BSR)
    return refuse(e, std::string("operator B is ") + kind_words(B.kind) + ": the build takes a BSR operator of the block size of A or the identity");
  if (!b_identity && B.sp.b != b)
    return refuse(e, "operator B is a BSR matrix of block size " + std::to_string(B.sp.b) + ", operator A of block size " + std::to_string(b) +
                         ": the build takes a BSR operator of the block size of A or the identity");
  const int64_t nb = e->n / b, bb = (int64_t)b * b;
  hipStream_t st = e->stream;
  Scratch sc(st);
  std::string why;
  // ---- the pattern of tril(A)^level over the block rows
  unsigned long long* bad = nullptr;
  int64_t* tile_sums = nullptr;
  sc.take(&bad, 1);
  sc.take(&tile_sums, (size_t)csr_build_scan_tiles(nb));
  if (sc.oom) return refuse(e, "device memory for the pattern could not be allocated");
  Pattern p1, pl;
  if (int rc = pattern_level(e, sc, A.sp, nb, b, 1, nullptr, nullptr, bad, tile_sums, &p1, &why)) return why.empty() ? unset(e, rc) : refuse(e, why);
  pl = p1;
  for (int l = 2; l <= level; ++l) {
    Pattern next;
    if (int rc = pattern_level(e, sc, A.sp, nb, b, l, &pl, &p1, bad, tile_sums, &next, &why)) return why.empty() ? unset(e, rc) : refuse(e, why);
    pl = next;
  }
  // ---- the block rows of G
  unsigned long long* lengths = nullptr;          // the longest block row and the classes that exist: three words come back
  sc.take(&lengths, 3);
  if (sc.oom) return refuse(e, "device memory for the pattern could not be allocated");
  unsigned long long hlen[3] = {0, 0, 0};
  if (int rc = row_lengths(st, pl.rp, nb, b, lengths, hlen)) return unset(e, rc);
  const int64_t longest = (int64_t)hlen[0];
  const bool small = hlen[1] != 0, large = hlen[2] != 0;
  if (pl.nnz >= ((int64_t)1 << 31)) return refuse(e, "G would hold 2^31 blocks or more");
  double *gval = nullptr, *tval = nullptr;
  int32_t *grow = nullptr, *tcol = nullptr;
  int64_t *trp = nullptr, *cursor = nullptr, *slot = nullptr;
  sc.take(&gval, (size_t)(pl.nnz * bb));
  sc.take(&grow, (size_t)pl.nnz);
  sc.take(&tval, (size_t)(pl.nnz * bb));
  sc.take(&tcol, (size_t)pl.nnz);
  sc.take(&slot, (size_t)pl.nnz);
  sc.take(&trp, (size_t)nb + 1);
  sc.take(&cursor, (size_t)nb);
  if (sc.oom) return refuse(e, "device memory for the " + std::to_string(pl.nnz) + " blocks of G could not be allocated");
  if (hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), st) != hipSuccess) return unset(e, fail(std::string(NAME) + ": hipMemsetAsync failed"));
  launch_bfsai_rows(st, pl.rp, pl.col, nb, b, A.sp.rp, A.sp.col, A.sp.val, b_identity ? nullptr : B.sp.rp, b_identity ? nullptr : B.sp.col,
                    b_identity ? nullptr : B.sp.val, sigma, small, large, gval, grow, bad);
  unsigned long long first_bad = 0;
  if (int rc = readback(st, &first_bad, bad, sizeof(first_bad))) return unset(e, rc);
  if (first_bad != ~0ull)
    return refuse(e, "A - sigma B is not positive definite on the pattern of block row " + std::to_string((int64_t)first_bad));
  // ---- the block rows of G^T: offsets by block column, a slot per block, the blocks copied untouched
  if (hipMemsetAsync(trp, 0, sizeof(int64_t) * ((size_t)nb + 1), st) != hipSuccess ||
      hipMemsetAsync(cursor, 0, sizeof(int64_t) * (size_t)nb, st) != hipSuccess)
    return unset(e, fail(std::string(NAME) + ": hipMemsetAsync failed"));
  launch_bfsai_transpose_count(st, pl.col, pl.nnz, trp + 1);
  launch_csr_build_scan(st, trp + 1, nb, tile_sums);
  launch_bfsai_transpose_fill(st, pl.col, grow, gval, pl.nnz, b, trp, cursor, slot, tcol, tval);
  if (hipGetLastError() != hipSuccess) return unset(e, fail(std::string(NAME) + ": a launch failed"));
  // ---- the two stores, both by the device BSR build: G from its row-major blocks, G^T from the same blocks read column-major
  OpDesc& M = e->op[DAV_OP_M];
  const int keep_map = e->keep_map[DAV_OP_M];
  e->keep_map[DAV_OP_M] = 0;
  int rc = dav_set_operator_bsr_dev(e, DAV_OP_M, b, pl.rp, 64, pl.col, 32, gval, 0, DAV_CSR_FULL, DAV_BSR_ROW_MAJOR);
  SparseStore g;
  if (rc == 0) {          // the first store is parked while the second is built
    g = M.sp;
    M.sp = SparseStore();
    M.kind = DAV_KIND_NONE;
    rc = dav_set_operator_bsr_dev(e, DAV_OP_M, b, trp, 64, tcol, 32, tval, 0, DAV_CSR_FULL, DAV_BSR_COL_MAJOR);
  }
  e->keep_map[DAV_OP_M] = keep_map;
  if (rc != 0) {          // the entry refused (device memory): its message, under this entry's name; slot M is unset
    const std::string inner = dav_last_error();
    (void)hipStreamSynchronize(st);
    sparse_store_release(g);
    return refuse(e, "the stores of G could not be built (" + inner + ")");
  }
  if (int rc2 = row_lengths(st, M.sp.rp, nb, b, lengths, hlen)) {
    (void)hipStreamSynchronize(st);
    sparse_store_release(g);
    return unset(e, rc2);
  }
  M.sp2 = M.sp;
  M.sp = g;
  M.fsai_longest_row = longest;
  M.fsai_longest_col = (int64_t)hlen[0];
  M.kind = DAV_KIND_BFSAI;
  e->diag_host[DAV_OP_M].clear();          // the diagonal of a preconditioner is never read: none is kept
  return 0;
}

extern "C" int davq_block_fsai_info(dav_handle_t e, int* block_size, int64_t* nnzb, int64_t* longest_row, int64_t* longest_col) {
  if (!e) return fail("davq_block_fsai_info: null engine");
  const OpDesc& M = e->op[DAV_OP_M];
  const bool built = M.kind == DAV_KIND_BFSAI;
  if (block_size) *block_size = built ? M.sp.b : 0;
  if (nnzb) *nnzb = built ? M.sp.nnz : 0;
  if (longest_row) *longest_row = built ? M.fsai_longest_row : 0;
  if (longest_col) *longest_col = built ? M.fsai_longest_col : 0;
  return 0;
}

extern "C" int davq_block_fsai_get_factor(dav_handle_t e, int transposed, int64_t* block_row_ptr, int32_t* block_col_idx, double* vals) {
  if (!e) return fail("davq_block_fsai_get_factor: null engine");
  CHK(bind(e));
  const OpDesc& M = e->op[DAV_OP_M];
  if (M.kind != DAV_KIND_BFSAI)
    return fail(std::string("davq_block_fsai_get_factor: slot DAV_OP_M is ") + kind_words(M.kind) + ", not a built block FSAI preconditioner");
  if (!block_row_ptr || !block_col_idx || !vals) return fail("davq_block_fsai_get_factor: null block_row_ptr, block_col_idx or vals");
  const SparseStore& s = transposed ? M.sp2 : M.sp;
  const int b = s.b;
  CHK(readback(e->stream, block_row_ptr, s.rp, sizeof(int64_t) * ((size_t)(e->n / b) + 1)));
  if (s.nnz > 0) {
    CHK(readback(e->stream, block_col_idx, s.col, sizeof(int32_t) * (size_t)s.nnz));
    CHK(readback(e->stream, vals, s.val, sizeof(double) * (size_t)s.nnz * b * b));
    for (int64_t p = 0; p < s.nnz; ++p) {          // the store keeps its blocks column-major: moved to row-major, never computed with
      double* blk = vals + p * b * b;
      for (int r = 0; r < b; ++r)
        for (int c = r + 1; c < b; ++c) std::swap(blk[r * b + c], blk[c * b + r]);
    }
  }
  return 0;
}
