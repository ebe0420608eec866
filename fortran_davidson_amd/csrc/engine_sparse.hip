// Engine, sparse operators: a symmetric matrix in CSR or BSR form, given in host arrays (dav_set_operator_csr, dav_set_operator_bsr) or in
// device arrays and built on the GPU (dav_set_operator_csr_dev, dav_set_operator_bsr_dev; kernels in k_csr_build.hip, k_bsr_build.hip);
// a CSR matrix also as unordered COO triples (davx_set_operator_coo, davx_set_operator_coo_dev; k_coo_build.hip).
// A complex Hermitian CSR matrix goes in as the BSR matrix of its 2 x 2 real blocks, its (re, im) values read where they lie
// (davh_set_operator_csr, davh_set_operator_csr_dev; the pair kernels of k_bsr_build.hip).
// All four entries follow one structure: the PATTERN - row_ptr and col_idx over rows or block rows - is validated; the
// canonical order of this rank's rows is built with a PAYLOAD per column index (CSR: the value of the entry; BSR: the source of the block,
// input position << 1 | mirrored); BSR gathers the VALUES from the sources; the DIAGONAL is summed per kind; one COMMIT step builds the
// work list and sets the operator.  Host and device entries produce the same arrays bit for bit.  With dav_keep_value_map on, CSR travels
// with sources too and every entry keeps them (the value map) with the sources of the diagonal; dav_update_operator_values(_dev) then
// repeats the VALUES and DIAGONAL steps alone on new numbers (kernels in k_sparse_refresh.hip).
// DAV_CSR_DIAGONALS or-ed into the triangle of a CSR entry: the entry decides from the offsets of the whole matrix
// whether it suits the storage by diagonals (dia_rule.h) before it builds anything, builds the canonical CSR as always, and a last step
// moves the values into the diagonals (k_dia.hip) and releases the canonical arrays - unless the value map is kept: then rp / col / val
// stay for the refresh, which fills the diagonals again (device memory: that of the CSR operator with its map plus 8 nd nloc bytes).
#include "engine_internal.h"
#include "dia_rule.h"
#include "coo_host.h"
#include "davidson_hip_ext.h"
#include "davidson_hip_herm.h"

static bool sparse_store_empty(const SparseStore& s) {
  return !s.rp && !s.col && !s.val && !s.items && !s.longs && !s.part && !s.src && !s.doff && !s.dpos && !s.bdiag && !s.rbound && !s.dia_off && !s.dia_val;
}
void sparse_store_release(SparseStore& s) {
  pool_free(s.rp); pool_free(s.col); pool_free(s.val);
  pool_free(s.items); pool_free(s.longs); pool_free(s.part);
  pool_free(s.src); pool_free(s.doff); pool_free(s.dpos);
  pool_free(s.bdiag);
  pool_free(s.rbound);
  pool_free(s.dia_off); pool_free(s.dia_val);
  s = SparseStore();
}
void sparse_release(E* e, OpDesc& o) {
  if (sparse_store_empty(o.sp) && sparse_store_empty(o.sp2) && !o.fsai_ws) return;
  (void)hipStreamSynchronize(e->stream);         // applies in flight may still read the arrays
  sparse_store_release(o.sp);
  sparse_store_release(o.sp2);                   // DAV_KIND_FSAI / DAV_KIND_BFSAI: the rows of G^T and the block between the two products
  pool_free(o.fsai_ws);
  o.fsai_ws = nullptr;
  o.fsai_longest_row = o.fsai_longest_col = 0;
}

// the one table of the kinds in words: the refusals of BDPR, CHEB / LCHEB and davp_build_fsai that name what an operator is
const char* kind_words(int kind) {
  switch (kind) {
    case DAV_KIND_NONE: return "not set";
    case DAV_KIND_DENSE: return "a dense matrix";
    case DAV_KIND_IDENTITY: return "the identity";
    case DAV_KIND_HOST: return "a host callback";
    case DAV_KIND_DEVICE: return "a device callback";
    case DAV_KIND_CSR: return "a CSR matrix";
    case DAV_KIND_BSR: return "a BSR matrix";
    case DAV_KIND_DIA: return "a CSR matrix stored by diagonals";
    case DAV_KIND_FSAI: return "a built FSAI preconditioner (DAV_KIND_FSAI)";
    case DAV_KIND_BFSAI: return "a built block FSAI preconditioner (DAV_KIND_BFSAI)";
    default: return "a generated operator";
  }
}

namespace {
// Work list of the block product over the canonical local rows (block rows) rp[0..nrows]: runs of at most max_rows whole rows with at most
// chunk entries (blocks) together, and every row longer than chunk cut into chunks at multiples of chunk from its first entry (one item
// and one partial slot each; CsrLong lists the slots of the row).  The cut depends on the row alone, so the sums do not depend on the ranks.
void sparse_build_items(const std::vector<int64_t>& rp, int max_rows, int64_t chunk, std::vector<CsrItem>& items, std::vector<CsrLong>& longs,
                        int* nslots) {
  const int64_t nrows = (int64_t)rp.size() - 1;
  CsrItem cur{0, 0, 0, 0, -1, 0};
  int slots = 0;
  auto flush = [&]() { if (cur.nrows > 0) items.push_back(cur); cur.nrows = 0; };
  for (int64_t i = 0; i < nrows; ++i) {
    const int64_t a = rp[(size_t)i], z = rp[(size_t)i + 1];
    if (z - a > chunk) {
      flush();
      const int first = slots;
      for (int64_t q = a; q < z; q += chunk) items.push_back({q, std::min(z, q + chunk), (int32_t)i, 1, slots++, 0});
      longs.push_back({(int32_t)i, first, slots - first, 0});
      continue;
    }
    if (cur.nrows > 0 && (cur.nrows == max_rows || z - cur.p0 > chunk)) flush();
    if (cur.nrows == 0) { cur.p0 = a; cur.row = (int32_t)i; }
    cur.p1 = z;
    cur.nrows += 1;
  }
  flush();
  *nslots = slots;
}

// ---- messages: every text exists once, composed from the nouns of the kind ---------------------------------------------------------------
struct SparseWords { const char *rp, *ci, *row, *rows, *col, *item, *items; };
const SparseWords CSR_WORDS{"row_ptr", "col_idx", "row", "rows", "column index", "entry", "entries"};
const SparseWords COO_WORDS{"row_idx", "col_idx", "row", "rows", "column index", "entry", "entries"};      // triples: rp names the row indices
const SparseWords BSR_WORDS{"block_row_ptr", "block_col_idx", "block row", "block rows", "block column", "block", "blocks"};

// one call of one of the four entries
struct Entry {
  E* e; int which; const char* name; const SparseWords& w;
  // a call that fails leaves the operator unset (the engine stays usable: set it again)
  int refuse(const std::string& msg) const {
    sparse_release(e, e->op[which]);
    e->op[which].kind = DAV_KIND_NONE;
    e->diag_host[which].clear();
    if (which == DAV_OP_A) e->basis_order.clear();
    return fail(std::string(name) + ": " + msg);
  }
  // the outcome of a build step: non-zero with a reason (the matrix is refused with it) or without (a HIP failure, already recorded by fail())
  int step(int rc, const std::string& why) const { return why.empty() ? rc : refuse(why); }
};

int entry_begin(E* e, int which, const char* name) {
  if (!e) return fail(std::string(name) + ": null engine");
  if (which < 0 || which >= N_OPS) return fail(std::string(name) + ": bad operator id");
  return bind(e);
}

// the scalar arguments, before anything is read, allocated or launched ("" = fine).  bsr: b and block_layout count (a CSR entry passes
// neither); bits = {row_ptr_bits, col_bits} of a device entry, nullptr for a host entry
std::string bad_arguments(const SparseWords& w, int64_t n, bool bsr, int b, int index_base, int triangle, int block_layout, const int* bits,
                          const void* row_ptr) {
  if (!bsr) {
    if (n >= ((int64_t)1 << 31)) return "n = " + std::to_string(n) + " must be below 2^31 (int32 column indices)";
  } else {
    if (b < 1 || b > 16) return "block_size = " + std::to_string(b) + " must lie in 1..16";
    if (n % b != 0) return "n = " + std::to_string(n) + " is not a multiple of block_size = " + std::to_string(b);
    if (n / b >= ((int64_t)1 << 31)) return "n / block_size must be below 2^31 (int32 block columns)";
  }
  if (index_base != 0 && index_base != 1) return "index_base must be 0 or 1";
  if ((triangle & ~(DAV_CSR_LOWER | DAV_CSR_DIAGONALS)) != 0) return "triangle must be DAV_CSR_FULL or DAV_CSR_LOWER";
  if (bsr && (triangle & DAV_CSR_DIAGONALS)) return "DAV_CSR_DIAGONALS serves the CSR entries only (dav_set_operator_csr / dav_set_operator_csr_dev): a BSR matrix is not stored by diagonals";
  if (bsr && block_layout != DAV_BSR_ROW_MAJOR && block_layout != DAV_BSR_COL_MAJOR) return "block_layout must be DAV_BSR_ROW_MAJOR or DAV_BSR_COL_MAJOR";
  if (bits && bits[0] != 32 && bits[0] != 64) return "row_ptr_bits must be 32 or 64";
  if (bits && bits[1] != 32 && bits[1] != 64) return "col_bits must be 32 or 64";
  if (!row_ptr) return std::string("null ") + w.rp;
  return "";
}

std::string msg_first_offset(const SparseWords& w, int64_t rp0, int base) {
  return std::string(w.rp) + "[0] = " + std::to_string(rp0) + " must equal the index base " + std::to_string(base);
}
std::string msg_decreases(const SparseWords& w, int64_t row) { return std::string(w.rp) + " decreases at " + w.row + " " + std::to_string(row); }
std::string msg_null_entries(const SparseWords& w) { return std::string("null ") + w.ci + " or vals"; }
// entry p of row i (both from 0) carries the caller's column c: outside the matrix, or above the diagonal of a lower triangle
std::string msg_bad_entry(const SparseWords& w, int64_t n, int base, int64_t p, int64_t i, int64_t c) {
  if (c - base < 0 || c - base >= n)
    return std::string(w.col) + " " + std::to_string(c) + " out of range at " + w.item + " " + std::to_string(p + base) + " (" + w.row + " " +
           std::to_string(i + base) + ")";
  return std::string(w.item) + " (" + std::to_string(i + base) + ", " + std::to_string(c) + ") lies above the diagonal of a DAV_CSR_LOWER matrix";
}
// triple p (from 0) carries the caller's row r and column c: the row outside the matrix, or what msg_bad_entry says of the column
std::string msg_bad_triple(const SparseWords& w, int64_t n, int base, int64_t p, int64_t r, int64_t c) {
  if (r - base < 0 || r - base >= n)
    return std::string(w.row) + " index " + std::to_string(r) + " out of range at " + w.item + " " + std::to_string(p + base);
  return msg_bad_entry(w, n, base, p, r - base, c);
}
// the scalar arguments of a COO entry ("" = fine; coo_host.h); bits = {row_bits, col_bits} of the device entry, nullptr for the host entry
std::string bad_triples(int64_t n, int64_t nnz, int index_base, int triangle, const int* bits, const void* row_idx, const void* col_idx,
                        const void* vals) {
  return coo_bad_arguments(n, nnz, index_base, triangle, DAV_CSR_LOWER | DAV_CSR_DIAGONALS, bits, row_idx, col_idx, vals);
}
std::string no_memory(const std::string& what) { return "device memory for " + what + " could not be allocated"; }
// (the estimates of the entries differ: 12 lnnz + 8 nloc bytes for CSR, 8 b^2 + 4 per block from host arrays, 8 b^2 + 12 from device arrays)
std::string stored(const SparseWords& w, int64_t count, int64_t bytes) {
  return std::to_string(count) + " " + w.items + " of this rank (" + std::to_string(bytes >> 20) + " MiB)";
}
std::string work_list(const SparseWords& w, int64_t count) { return "the work list of " + std::to_string(count) + " " + w.items + " of this rank"; }

// ---- storage that stays with the operator -------------------------------------------------------------------------------------------------
template <class T> bool keep(T** p, size_t count) {
  if (pool_malloc(p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
  return true;
}
template <class T> bool upload(T** dst, const std::vector<T>& src) {
  if (!keep(dst, src.size())) return false;
  if (!src.empty() && hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}

int readback(hipStream_t st, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// The last step of every entry, with rp / col / val of the store in place: the diagonal (of the whole matrix: diag on the host, or diag_dev
// on the device, read back into diag), the work list over the canonical offsets rp, and the operator's description.  oom: the entry's
// words for a failed allocation.
int sparse_commit(const Entry& en, int kind, int b, int64_t grow0, const std::vector<int64_t>& rp, std::vector<double>& diag, const double* diag_dev,
                  const std::string& oom) {
  E* e = en.e;
  OpDesc& o = e->op[en.which];
  SparseStore& s = o.sp;
  if (diag_dev) {
    if (e->nloc > 0) HIPCHK(hipMemcpyAsync(o.diag, diag_dev + e->row0, sizeof(double) * e->nloc, hipMemcpyDeviceToDevice, e->stream));
    diag.resize((size_t)e->n);
    CHK(readback(e->stream, diag.data(), diag_dev, sizeof(double) * (size_t)e->n));
  } else if (e->nloc > 0) {
    HIPCHK(hipMemcpy(o.diag, diag.data() + e->row0, sizeof(double) * e->nloc, hipMemcpyHostToDevice));
  }
  const bool csr = kind == DAV_KIND_CSR;
  std::vector<CsrItem> items;
  std::vector<CsrLong> longs;
  int nslots = 0;
  sparse_build_items(rp, csr ? CSR_ROWS : std::max(1, BSR_ROWS / b), csr ? CSR_CHUNK : BSR_CHUNK, items, longs, &nslots);
  if (!upload(&s.items, items) || !upload(&s.longs, longs) || !keep(&s.part, (size_t)nslots * (csr ? 64 : 1024))) return en.refuse(oom);
  HIPCHK(hipStreamSynchronize(e->stream));          // the caller's arrays are free again when the call returns
  HIPCHK(hipGetLastError());
  s.nitems = (int)items.size();
  s.nlong = (int)longs.size();
  s.nnz = rp.back();
  s.nrows = (int64_t)rp.size() - 1;
  s.b = b;
  s.grow0 = grow0;
  o.storage = 0;
  e->diag_host[en.which].swap(diag);
  if (en.which == DAV_OP_A) e->basis_order.clear();
  o.kind = kind;
  return 0;
}

// the block rows [ib0, ib0 + nbl) that touch this rank's slab [row0, row0 + nloc)
void local_block_rows(const E* e, int b, int64_t* ib0, int64_t* nbl) {
  *ib0 = e->nloc > 0 ? e->row0 / b : 0;
  *nbl = e->nloc > 0 ? (e->row0 + e->nloc + b - 1) / b - *ib0 : 0;
}

// ---- host arrays ------------------------------------------------------------------------------------------------------------------------
// the caller's pattern: n rows (block rows) of the whole matrix, of which [r0, r0 + nloc) are this rank's
struct HostPattern {
  const int64_t* row_ptr; const int32_t* col_idx;
  int64_t n, r0, nloc;
  int base; bool lower;
};

// row_ptr first, then the entries: the first offending position
bool pattern_validate(const HostPattern& P, const void* vals, const SparseWords& w, std::string* why) {
  const int64_t* g = P.row_ptr;
  if (g[0] != P.base) { *why = msg_first_offset(w, g[0], P.base); return false; }
  for (int64_t i = 0; i < P.n; ++i)
    if (g[i + 1] < g[i]) { *why = msg_decreases(w, i + P.base); return false; }
  if (g[P.n] - P.base > 0 && (!P.col_idx || !vals)) { *why = msg_null_entries(w); return false; }
  for (int64_t i = 0; i < P.n; ++i)
    for (int64_t p = g[i] - P.base; p < g[i + 1] - P.base; ++p) {
      const int64_t j = (int64_t)P.col_idx[p] - P.base;
      if (j < 0 || j >= P.n || (P.lower && j > i)) { *why = msg_bad_entry(w, P.n, P.base, p, i, P.col_idx[p]); return false; }
    }
  return true;
}

// Canonical rows of this rank: own entries in input order, then (lower) the mirrored strict lower entries in the order of their source rows;
// stable sort by column (duplicates stay separate terms, in that order).  payload(p, mirrored) is what travels with the column of input entry p.
template <class V, class F>
void pattern_order(const HostPattern& P, F payload, std::vector<int64_t>& rp, std::vector<int32_t>& lcol, std::vector<V>& lpay) {
  const int64_t* g = P.row_ptr;
  const int64_t r0 = P.r0, nloc = P.nloc, base = P.base;
  auto each_mirrored = [&](auto&& f) {         // f(i, j, p): entry p of row i lies below the diagonal and its mirror image in local row j
    if (!P.lower) return;
    for (int64_t i = 0; i < P.n; ++i)
      for (int64_t p = g[i] - base; p < g[i + 1] - base; ++p) {
        const int64_t j = (int64_t)P.col_idx[p] - base;
        if (j < i && j >= r0 && j < r0 + nloc) f(i, j, p);
      }
  };
  rp.assign((size_t)nloc + 1, 0);
  for (int64_t i = r0; i < r0 + nloc; ++i) rp[(size_t)(i - r0) + 1] = g[i + 1] - g[i];
  each_mirrored([&](int64_t, int64_t j, int64_t) { rp[(size_t)(j - r0) + 1] += 1; });
  for (int64_t i = 0; i < nloc; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
  lcol.resize((size_t)rp[(size_t)nloc]);
  lpay.resize((size_t)rp[(size_t)nloc]);
  std::vector<int64_t> pos(rp.begin(), rp.end() - 1);
  for (int64_t i = r0; i < r0 + nloc; ++i)
    for (int64_t p = g[i] - base; p < g[i + 1] - base; ++p) {
      const size_t q = (size_t)pos[(size_t)(i - r0)]++;
      lcol[q] = (int32_t)(P.col_idx[p] - base);
      lpay[q] = payload(p, false);
    }
  each_mirrored([&](int64_t i, int64_t j, int64_t p) {
    const size_t q = (size_t)pos[(size_t)(j - r0)]++;
    lcol[q] = (int32_t)i;
    lpay[q] = payload(p, true);
  });
  std::vector<std::pair<int32_t, V>> row;
  for (int64_t i = 0; i < nloc; ++i) {
    const size_t a = (size_t)rp[(size_t)i], z = (size_t)rp[(size_t)i + 1];
    if (std::is_sorted(lcol.begin() + a, lcol.begin() + z)) continue;
    row.clear();
    for (size_t q = a; q < z; ++q) row.push_back({lcol[q], lpay[q]});
    std::stable_sort(row.begin(), row.end(), [](const std::pair<int32_t, V>& x, const std::pair<int32_t, V>& y) { return x.first < y.first; });
    for (size_t q = a; q < z; ++q) { lcol[q] = row[q - a].first; lpay[q] = row[q - a].second; }
  }
}

// What a set call made with dav_keep_value_map on keeps besides the operator, as a host entry builds it: the value map of this rank's
// entries (blocks) and the diagonal sources of the whole matrix (SparseStore::src, doff, dpos); gcount / triangle / rowmaj describe the
// caller's vals.
struct HostMap {
  std::vector<uint64_t> src;
  std::vector<int64_t> doff, dpos;
  int64_t gcount = 0;
  int triangle = 0, rowmaj = 0, pairs = 0, base = 0;
};
std::string map_memory(const SparseWords& w) { return no_memory(std::string("the value map of the ") + w.items + " of this rank"); }

// the canonical arrays to the device (the engine's allocator; released when the operator is set again and at dav_destroy), then the commit
int commit_host(const Entry& en, int kind, int b, int64_t grow0, const std::vector<int64_t>& rp, const std::vector<int32_t>& lcol,
                const std::vector<double>& lval, std::vector<double>& diag, int64_t bytes, const HostMap* map) {
  CHK(operator_goes(en.e, en.which, true));
  SparseStore& s = en.e->op[en.which].sp;
  const std::string oom = no_memory(stored(en.w, rp.back(), bytes));
  if (!upload(&s.rp, rp) || !upload(&s.col, lcol) || !upload(&s.val, lval)) return en.refuse(oom);
  if (map) {
    if (!upload(&s.src, map->src) || !upload(&s.doff, map->doff) || !upload(&s.dpos, map->dpos)) return en.refuse(map_memory(en.w));
    s.gcount = map->gcount; s.triangle = map->triangle; s.rowmaj = map->rowmaj; s.pairs = map->pairs; s.pairs_base = map->base;
  }
  return sparse_commit(en, kind, b, grow0, rp, diag, nullptr, oom);
}

// ---- storage by diagonals (DAV_CSR_DIAGONALS) ---------------------------------------------------------------------------------------------
// the offsets of the whole matrix from its marks and the rule of dia_rule.h; false: *why says what the matrix has and what the rule asks
bool dia_decide(const uint8_t* marks, int64_t n, int64_t nnz, int64_t ndiag, bool lower, std::vector<int32_t>& offs, std::string* why) {
  dia_offsets_from_marks(marks, n, offs);
  const int64_t entries = dia_canonical_entries(nnz, ndiag, lower);
  if (dia_eligible((int64_t)offs.size(), n, entries)) return true;
  *why = dia_refusal((int64_t)offs.size(), n, entries);
  return false;
}

// the slots of this rank from its canonical rows (rp / col / val of the store, on the device)
void dia_fill(E* e, const SparseStore& s) {
  launch_dia_fill(e->stream, s.rp, s.col, s.val, e->nloc, e->row0, s.dia_off, s.dia_nd, s.dia_val, s.dia_ld);
}

// The last step of a CSR entry called with DAV_CSR_DIAGONALS, behind the commit: the diagonals are allocated and filled, the operator
// becomes DAV_KIND_DIA and what only the CSR product reads is released (with the value map kept: the work list alone).
int dia_commit(const Entry& en, const std::vector<int32_t>& offs) {
  E* e = en.e;
  OpDesc& o = e->op[en.which];
  SparseStore& s = o.sp;
  s.dia_nd = (int)offs.size();
  s.dia_ld = dia_leading_dimension(e->nloc);
  const size_t slots = (size_t)s.dia_nd * (size_t)s.dia_ld;
  if (!upload(&s.dia_off, offs) || !keep(&s.dia_val, slots))
    return en.refuse(no_memory(std::to_string(s.dia_nd) + " diagonals of this rank (" + std::to_string((8 * slots) >> 20) + " MiB)"));
  dia_fill(e, s);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  pool_free(s.items); pool_free(s.longs); pool_free(s.part);
  s.items = nullptr; s.longs = nullptr; s.part = nullptr;
  s.nitems = 0; s.nlong = 0;
  if (!s.src) {
    pool_free(s.rp); pool_free(s.col); pool_free(s.val);
    s.rp = nullptr; s.col = nullptr; s.val = nullptr;
  }
  o.kind = DAV_KIND_DIA;
  return 0;
}
}  // namespace

namespace {
// The host CSR path behind dav_set_operator_csr and davx_set_operator_coo.  perm (COO: the row form is a permutation of the caller's
// triples) = the caller's position of every entry of vals; the value map and the diagonal sources then name the caller's positions.
int set_csr_host(const Entry& en, const int64_t* row_ptr, const int32_t* col_idx, const double* vals, int index_base, int triangle,
                 const int64_t* perm) {
  E* e = en.e;
  const int which = en.which;
  const int64_t n = e->n;
  std::string why = bad_arguments(en.w, n, false, 0, index_base, triangle, 0, nullptr, row_ptr);
  if (!why.empty()) return en.refuse(why);
  const HostPattern P{row_ptr, col_idx, n, e->row0, e->nloc, index_base, (triangle & DAV_CSR_LOWER) != 0};
  if (!pattern_validate(P, vals, en.w, &why)) return en.refuse(why);
  std::vector<int32_t> dia_offsets;
  if (triangle & DAV_CSR_DIAGONALS) {
    std::vector<uint8_t> marks;
    int64_t ndiag = 0;
    dia_mark_host(row_ptr, col_idx, n, index_base, P.lower, marks, &ndiag);
    if (!dia_decide(marks.data(), n, row_ptr[n] - index_base, ndiag, P.lower, dia_offsets, &why)) return en.refuse(why);
  }
  std::vector<int64_t> rp;
  std::vector<int32_t> lcol;
  std::vector<double> lval;
  const bool keep_map = e->keep_map[which] != 0;
  HostMap map;
  if (keep_map) {          // the order with the source of an entry as payload (as BSR has it); the values then follow their sources
    pattern_order(P, [](int64_t p, bool mirrored) { return (uint64_t)p << 1 | (uint64_t)mirrored; }, rp, lcol, map.src);
    lval.resize(map.src.size());
    for (size_t q = 0; q < lval.size(); ++q) lval[q] = vals[map.src[q] >> 1];
    map.doff.assign((size_t)n + 1, 0);
    map.gcount = row_ptr[n] - index_base;
    map.triangle = triangle & DAV_CSR_LOWER;
  } else {
    pattern_order(P, [&](int64_t p, bool) { return vals[p]; }, rp, lcol, lval);
  }
  // the diagonal of the whole matrix, from the global arrays: duplicates summed in input order, a missing entry counts as 0
  std::vector<double> diag((size_t)n, 0.0);
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t p = row_ptr[i] - index_base; p < row_ptr[i + 1] - index_base; ++p)
      if ((int64_t)col_idx[p] - index_base == i) {
        diag[(size_t)i] += vals[p];
        if (keep_map) map.dpos.push_back(p);
      }
    if (keep_map) map.doff[(size_t)i + 1] = (int64_t)map.dpos.size();
  }
  if (keep_map && perm) {
    for (uint64_t& q : map.src) q = (uint64_t)perm[q >> 1] << 1 | (q & 1);
    for (int64_t& p : map.dpos) p = perm[p];
  }
  CHK(commit_host(en, DAV_KIND_CSR, 1, 0, rp, lcol, lval, diag, 12 * rp.back() + 8 * e->nloc, keep_map ? &map : nullptr));
  return (triangle & DAV_CSR_DIAGONALS) ? dia_commit(en, dia_offsets) : 0;
}
}  // namespace

extern "C" int dav_set_operator_csr(dav_handle_t e, int which, const int64_t* row_ptr, const int32_t* col_idx, const double* vals,
                                    int index_base, int triangle) {
  CHK(entry_begin(e, which, "dav_set_operator_csr"));
  return set_csr_host(Entry{e, which, "dav_set_operator_csr", CSR_WORDS}, row_ptr, col_idx, vals, index_base, triangle, nullptr);
}

// COO triples in host memory: validated in the order of the triples (the first offending p is named), brought into their row form by a
// stable counting sort on the row, and from there the host CSR path - with the positions of the triples in the value map.
extern "C" int davx_set_operator_coo(dav_handle_t e, int which, int64_t nnz, const int32_t* row_idx, const int32_t* col_idx, const double* vals,
                                    int index_base, int triangle) {
  CHK(entry_begin(e, which, "davx_set_operator_coo"));
  const Entry en{e, which, "davx_set_operator_coo", COO_WORDS};
  const int64_t n = e->n;
  const std::string why = bad_triples(n, nnz, index_base, triangle, nullptr, row_idx, col_idx, vals);
  if (!why.empty()) return en.refuse(why);
  const int64_t bad = coo_first_bad(n, nnz, row_idx, col_idx, index_base, (triangle & DAV_CSR_LOWER) != 0);
  if (bad >= 0) return en.refuse(msg_bad_triple(en.w, n, index_base, bad, row_idx[bad], col_idx[bad]));
  CooRowForm f;
  coo_row_form(n, nnz, row_idx, col_idx, vals, index_base, f);
  const int32_t none_i = 0;
  const double none_v = 0.0;
  return set_csr_host(en, f.row_ptr.data(), nnz > 0 ? f.col.data() : &none_i, nnz > 0 ? f.val.data() : &none_v, index_base, triangle,
                      f.perm.data());
}

namespace {
// ---- the (re, im) value source: a complex Hermitian CSR matrix as the BSR matrix of its 2 x 2 blocks (davh_*) ----------
// the scalar arguments of a davh_ entry ("" = fine): the real order even, then what a CSR entry asks of the order n / 2
std::string bad_arguments_herm(const SparseWords& w, int64_t n, int index_base, int triangle, const int* bits, const void* row_ptr) {
  if (n % 2 != 0)
    return "n = " + std::to_string(n) + " is odd: a Hermitian operator of order n / 2 needs an engine of the even real order n (re, im interleaved)";
  const std::string why = bad_arguments(w, n / 2, false, 0, index_base, triangle, 0, bits, row_ptr);
  if (!why.empty()) return why;
  if (triangle & DAV_CSR_DIAGONALS) return "DAV_CSR_DIAGONALS serves the real CSR entries only: a Hermitian operator is stored by blocks";
  return "";
}
// diagonal entry p of row i (both from 0) carries the imaginary part im: the real form would not be symmetric
std::string msg_imag_diagonal(const SparseWords& w, int base, int64_t p, int64_t i, double im) {
  char num[40];
  snprintf(num, sizeof num, "%.17g", im);
  return std::string("diagonal ") + w.item + " " + std::to_string(p + base) + " (" + w.row + " " + std::to_string(i + base) +
         ") has the imaginary part " + num + ": the diagonal of a Hermitian matrix is real";
}

// The host BSR path behind dav_set_operator_bsr and davh_set_operator_csr.  pairs: vals holds one (re, im) pair (a, b) per block, b = 2,
// standing for the row-major block [[a, -b], [b, a]]; the words and the scalar checks are the entry's own.
int set_bsr_host(const Entry& en, int b, const int64_t* block_row_ptr, const int32_t* block_col_idx, const double* vals, int index_base,
                 int triangle, int block_layout, bool pairs) {
  E* e = en.e;
  const int which = en.which;
  const int64_t n = e->n;
  std::string why;
  const int64_t nb = n / b, bb = (int64_t)b * b;
  int64_t ib0, nbl;
  local_block_rows(e, b, &ib0, &nbl);
  const HostPattern P{block_row_ptr, block_col_idx, nb, ib0, nbl, index_base, triangle == DAV_CSR_LOWER};
  if (!pattern_validate(P, vals, en.w, &why)) return en.refuse(why);
  if (pairs)
    for (int64_t I = 0; I < nb; ++I)
      for (int64_t p = block_row_ptr[I] - index_base; p < block_row_ptr[I + 1] - index_base; ++p)
        if ((int64_t)block_col_idx[p] - index_base == I && !(vals[2 * p + 1] == 0.0))
          return en.refuse(msg_imag_diagonal(en.w, index_base, p, I, vals[2 * p + 1]));
  std::vector<int64_t> rp;
  std::vector<int32_t> lcol;
  std::vector<uint64_t> src;        // source of each canonical block: input block p << 1 | mirrored
  pattern_order(P, [](int64_t p, bool mirrored) { return (uint64_t)p << 1 | (uint64_t)mirrored; }, rp, lcol, src);
  // entry (m, k) of input block p in the caller's layout
  const bool rowmaj = block_layout == DAV_BSR_ROW_MAJOR;
  auto entry = [&](int64_t p, int m, int k) {
    if (pairs) return m == k ? vals[2 * p] : m > k ? vals[2 * p + 1] : -vals[2 * p + 1];          // -b: a sign flip
    return vals[p * bb + (rowmaj ? (int64_t)m * b + k : (int64_t)k * b + m)];
  };
  // values column-major per block: lval[q * b * b + k * b + m] = A_q[m][k] (a mirrored block is the transpose of its source)
  std::vector<double> lval(src.size() * (size_t)bb);
  for (size_t q = 0; q < src.size(); ++q) {
    double* d = lval.data() + q * (size_t)bb;
    const int64_t p = (int64_t)(src[q] >> 1);
    const bool tr = src[q] & 1;
    for (int k = 0; k < b; ++k)
      for (int m = 0; m < b; ++m) d[(int64_t)k * b + m] = tr ? entry(p, k, m) : entry(p, m, k);
  }
  // the diagonal of the whole matrix, from the diagonal blocks of the global arrays (duplicates summed in input order)
  std::vector<double> diag((size_t)n, 0.0);
  const bool keep_map = e->keep_map[which] != 0;
  HostMap map;
  if (keep_map) {
    map.doff.assign((size_t)nb + 1, 0);
    map.gcount = block_row_ptr[nb] - index_base;
    map.triangle = triangle;
    map.rowmaj = rowmaj ? 1 : 0;
    map.pairs = pairs ? 1 : 0;
    map.base = index_base;
  }
  for (int64_t I = 0; I < nb; ++I) {
    for (int64_t p = block_row_ptr[I] - index_base; p < block_row_ptr[I + 1] - index_base; ++p)
      if ((int64_t)block_col_idx[p] - index_base == I) {
        for (int m = 0; m < b; ++m) diag[(size_t)(I * b + m)] += entry(p, m, m);
        if (keep_map) map.dpos.push_back(p);
      }
    if (keep_map) map.doff[(size_t)I + 1] = (int64_t)map.dpos.size();
  }
  if (keep_map) map.src.swap(src);          // the sources of the canonical blocks, as the order step left them
  return commit_host(en, DAV_KIND_BSR, b, ib0 * b - e->row0, rp, lcol, lval, diag, rp.back() * (8 * bb + 4), keep_map ? &map : nullptr);
}
}  // namespace

extern "C" int dav_set_operator_bsr(dav_handle_t e, int which, int block_size, const int64_t* block_row_ptr, const int32_t* block_col_idx,
                                    const double* vals, int index_base, int triangle, int block_layout) {
  CHK(entry_begin(e, which, "dav_set_operator_bsr"));
  const Entry en{e, which, "dav_set_operator_bsr", BSR_WORDS};
  const std::string why = bad_arguments(en.w, e->n, true, block_size, index_base, triangle, block_layout, nullptr, block_row_ptr);
  if (!why.empty()) return en.refuse(why);
  return set_bsr_host(en, block_size, block_row_ptr, block_col_idx, vals, index_base, triangle, block_layout, false);
}

// A complex Hermitian CSR matrix of order n / 2 in host arrays: the host BSR path with b = 2 over the caller's pattern, reading pairs.
extern "C" int davh_set_operator_csr(dav_handle_t e, int which, const int64_t* row_ptr, const int32_t* col_idx, const double* vals,
                                     int index_base, int triangle) {
  CHK(entry_begin(e, which, "davh_set_operator_csr"));
  const Entry en{e, which, "davh_set_operator_csr", CSR_WORDS};
  const std::string why = bad_arguments_herm(en.w, e->n, index_base, triangle, nullptr, row_ptr);
  if (!why.empty()) return en.refuse(why);
  return set_bsr_host(en, 2, row_ptr, col_idx, vals, index_base, triangle, DAV_BSR_ROW_MAJOR, true);
}

// ---- device arrays: the same steps on the GPU --------------------------------------------------------------------------------------------
// Both entries build the index level with the kernels of k_csr_build.hip - over the rows of a CSR matrix with the value of an entry as
// payload, over the block rows of a BSR matrix with the source of a block.  Each step returns 0, or non-zero with *why set (the caller
// refuses the matrix with that message) or *why empty (a HIP failure, already recorded by fail()).
// a caller's pointer: device memory of this engine's device, large enough where the runtime can tell (before any launch)
bool device_array(E* e, const void* p, const char* name, size_t bytes, std::string* why) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    *why = std::string(name) + " is not device memory (the runtime does not know the pointer)";
    return false;
  }
  if (at.type != hipMemoryTypeDevice) { *why = std::string(name) + " is not device memory (host, pinned or managed)"; return false; }
  if (at.device != e->device) {
    *why = std::string(name) + " lies on device " + std::to_string(at.device) + ", the engine on device " + std::to_string(e->device);
    return false;
  }
  hipDeviceptr_t lo = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&lo, &size, (hipDeviceptr_t)p) == hipSuccess) {
    if ((const char*)p + bytes > (const char*)lo + size)
      { *why = std::string(name) + " holds fewer than the " + std::to_string(bytes) + " bytes the matrix needs"; return false; }
  } else {
    (void)hipGetLastError();
  }
  return true;
}

namespace {
// scratch of a build: released on every way out, after the stream has finished with it
struct BuildScratch {
  hipStream_t st;
  std::vector<void*> held;
  bool oom = false;
  explicit BuildScratch(hipStream_t s) : st(s) {}
  BuildScratch(const BuildScratch&) = delete;
  ~BuildScratch() { (void)hipStreamSynchronize(st); for (void* p : held) pool_free(p); }
  template <class T> void take(T** p, size_t count) {
    *p = nullptr;
    if (oom) return;
    if (pool_malloc(p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; oom = true; return; }
    held.push_back((void*)*p);
  }
};

// the caller's pattern: n rows (block rows) of the whole matrix, of which [r0, r0 + nloc) are this rank's; item_bytes of vals per entry
struct DevPattern {
  const void* row_ptr; int rp64;
  const void* col_idx; int ci64;
  const double* vals; size_t item_bytes;
  int64_t n, r0, nloc;
  int base; bool lower;
  // set by pattern_validate_dev
  int64_t nnz = 0;
  int32_t* mcount = nullptr;               // mirrored entries per local row; later the slots taken by the scatter
  uint32_t* dcount = nullptr;              // diagonal entries per row of the whole matrix
  unsigned long long* dfirst = nullptr;    // the first of them
};

// the pointers, then the rules of pattern_validate on the device: row_ptr first, then the entries (the first offending position, as the host
// loop names it)
int pattern_validate_dev(E* e, BuildScratch& sc, DevPattern& P, const SparseWords& w, std::string* why) {
  hipStream_t st = e->stream;
  const size_t rpw = P.rp64 ? 8 : 4, ciw = P.ci64 ? 8 : 4;
  const int64_t n = P.n;
  if (!device_array(e, P.row_ptr, w.rp, rpw * (size_t)(n + 1), why)) return 1;
  if (P.col_idx && !device_array(e, P.col_idx, w.ci, 0, why)) return 1;
  if (P.vals && !device_array(e, P.vals, "vals", 0, why)) return 1;
  unsigned long long* info = nullptr;
  sc.take(&info, 4);
  if (sc.oom) { *why = no_memory("the validation"); return 1; }
  HIPCHK(hipMemsetAsync(info, 0xff, sizeof(unsigned long long) * 4, st));
  launch_csr_build_rows(st, P.row_ptr, P.rp64, n, info);
  unsigned long long hinfo[4];
  CHK(readback(st, hinfo, info, sizeof(hinfo)));
  const int64_t rp0 = (int64_t)hinfo[1], rpn = (int64_t)hinfo[2];
  if (rp0 != P.base) { *why = msg_first_offset(w, rp0, P.base); return 1; }
  if (hinfo[0] != ~0ull) { *why = msg_decreases(w, (int64_t)hinfo[0] + P.base); return 1; }
  P.nnz = rpn - P.base;
  if (P.nnz > 0 && (!P.col_idx || !P.vals)) { *why = msg_null_entries(w); return 1; }
  if (hinfo[3] != ~0ull) {
    *why = std::string(w.row) + " " + std::to_string((int64_t)hinfo[3] + P.base) + " holds 2^32 " + w.items + " or more";
    return 1;
  }
  if (P.nnz > 0 && (!device_array(e, P.col_idx, w.ci, ciw * (size_t)P.nnz, why) || !device_array(e, P.vals, "vals", P.item_bytes * (size_t)P.nnz, why)))
    return 1;
  int64_t* locate = nullptr;
  sc.take(&P.mcount, (size_t)P.nloc); sc.take(&P.dcount, (size_t)n); sc.take(&P.dfirst, (size_t)n); sc.take(&locate, 2);
  if (sc.oom) { *why = no_memory("the validation of " + std::to_string(n) + " " + w.rows); return 1; }
  HIPCHK(hipMemsetAsync(P.mcount, 0, sizeof(int32_t) * std::max<int64_t>(P.nloc, 1), st));
  HIPCHK(hipMemsetAsync(P.dcount, 0, sizeof(uint32_t) * std::max<int64_t>(n, 1), st));
  HIPCHK(hipMemsetAsync(P.dfirst, 0xff, sizeof(unsigned long long) * std::max<int64_t>(n, 1), st));
  launch_csr_build_check(st, P.row_ptr, P.rp64, P.col_idx, P.ci64, n, P.nnz, P.base, P.lower ? 1 : 0, P.r0, P.nloc, info + 3, P.mcount, P.dcount,
                         P.dfirst);
  CHK(readback(st, hinfo, info, sizeof(hinfo)));
  if (hinfo[3] != ~0ull) {
    const int64_t p = (int64_t)hinfo[3];
    launch_csr_build_locate(st, P.row_ptr, P.rp64, P.col_idx, P.ci64, n, P.base, p, locate);
    int64_t loc[2];
    CHK(readback(st, loc, locate, sizeof(loc)));
    *why = msg_bad_entry(w, n, P.base, p, loc[0], loc[1]);
    return 1;
  }
  return 0;
}

// *lrp (kept with the operator) and rp = the int64 offsets of the canonical local rows
int pattern_offsets_dev(E* e, BuildScratch& sc, const DevPattern& P, const SparseWords& w, int64_t** lrp, std::vector<int64_t>& rp, std::string* why) {
  int64_t* tile_sums = nullptr;
  sc.take(&tile_sums, (size_t)csr_build_scan_tiles(P.nloc));
  if (sc.oom || !keep(lrp, (size_t)P.nloc + 1)) { *why = no_memory(std::string("the ") + w.row + " offsets of this rank"); return 1; }
  launch_csr_build_offsets(e->stream, P.row_ptr, P.rp64, P.r0, P.nloc, P.mcount, *lrp, tile_sums);
  rp.assign((size_t)P.nloc + 1, 0);
  CHK(readback(e->stream, rp.data(), *lrp, sizeof(int64_t) * rp.size()));
  return 0;
}

void pattern_scatter(hipStream_t st, const DevPattern& P, int64_t p_lo, int64_t p_hi, const int64_t* lrp, int32_t* ocol, double* oval, uint32_t* tie) {
  launch_csr_build_scatter(st, P.row_ptr, P.rp64, P.col_idx, P.ci64, P.vals, P.n, p_lo, p_hi, P.base, P.lower ? 1 : 0, P.r0, P.nloc, lrp, P.mcount,
                           ocol, oval, tie);
}
void pattern_scatter(hipStream_t st, const DevPattern& P, int64_t p_lo, int64_t p_hi, const int64_t* lrp, int32_t* ocol, uint64_t* osrc, uint32_t* tie) {
  launch_csr_build_scatter(st, P.row_ptr, P.rp64, P.col_idx, P.ci64, P.n, p_lo, p_hi, P.base, P.lower ? 1 : 0, P.r0, P.nloc, lrp, P.mcount, ocol,
                           osrc, tie);
}

template <class V>
int pattern_sort_dev(E* e, BuildScratch& sc, const SparseWords& w, const int64_t* lrp, const std::vector<int64_t>& rp, int32_t* ocol, V* oval,
                     const uint32_t* tie, uint8_t* flag, std::string* why);

// the canonical order: columns to ocol and payloads (values / block sources) to oval, every local row in the order of pattern_order
template <class V>
int pattern_order_dev(E* e, BuildScratch& sc, const DevPattern& P, const SparseWords& w, const int64_t* lrp, const std::vector<int64_t>& rp,
                      int32_t* ocol, V* oval, std::string* why) {
  hipStream_t st = e->stream;
  const int64_t nloc = P.nloc, lnnz = rp[(size_t)nloc];
  const size_t rpw = P.rp64 ? 8 : 4;
  uint32_t* tie = nullptr;
  uint8_t* flag = nullptr;
  if (P.lower) sc.take(&tie, (size_t)lnnz);
  sc.take(&flag, (size_t)nloc);
  if (sc.oom) { *why = no_memory("sorting " + std::to_string(lnnz) + " " + w.items); return 1; }
  // own entries: those of the local rows; mirrored entries (lower): any row of the matrix may send some
  int64_t p_lo = 0, p_hi = P.nnz;
  if (!P.lower && nloc > 0) {
    int64_t ends[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
      const char* src = (const char*)P.row_ptr + rpw * (size_t)(s == 0 ? P.r0 : P.r0 + nloc);
      CHK(readback(st, &ends[s], src, rpw));
      if (!P.rp64) ends[s] = (int64_t)(int32_t)ends[s];
    }
    p_lo = ends[0] - P.base;
    p_hi = ends[1] - P.base;
  }
  HIPCHK(hipMemsetAsync(P.mcount, 0, sizeof(int32_t) * std::max<int64_t>(nloc, 1), st));
  if (nloc > 0) pattern_scatter(st, P, p_lo, p_hi, lrp, ocol, oval, tie);
  return pattern_sort_dev(e, sc, w, lrp, rp, ocol, oval, tie, flag, why);
}

// Rows lrp[0..nloc] (rp: the same offsets on the host) of columns ocol with payloads oval, each row into the order of its keys (column,
// tie; tie == nullptr: the position is the tie): rows out of order are flagged, those of at most one LDS tile sorted by one workgroup each,
// longer ones by tiles and merge passes.  flag: nloc bytes of scratch.
template <class V>
int pattern_sort_dev(E* e, BuildScratch& sc, const SparseWords& w, const int64_t* lrp, const std::vector<int64_t>& rp, int32_t* ocol, V* oval,
                     const uint32_t* tie, uint8_t* flag, std::string* why) {
  hipStream_t st = e->stream;
  const int64_t nloc = (int64_t)rp.size() - 1, lnnz = rp[(size_t)nloc];
  HIPCHK(hipMemsetAsync(flag, 0, std::max<int64_t>(nloc, 1), st));
  launch_csr_build_flag(st, lrp, nloc, lnnz, ocol, tie, flag);
  launch_csr_build_sort_rows(st, lrp, nloc, flag, ocol, oval, tie);
  // rows longer than one LDS tile that are out of order: tiles sorted, then merged (one row at a time)
  const int64_t tile = csr_build_sort_tile();
  int64_t longest = 0;
  std::vector<int64_t> cand, longs_unsorted;
  for (int64_t i = 0; i < nloc; ++i)
    if (rp[(size_t)i + 1] - rp[(size_t)i] > tile) cand.push_back(i);
  if (!cand.empty()) {
    std::vector<uint8_t> hflag((size_t)nloc);
    CHK(readback(st, hflag.data(), flag, (size_t)nloc));
    for (int64_t i : cand)
      if (hflag[(size_t)i]) { longs_unsorted.push_back(i); longest = std::max(longest, rp[(size_t)i + 1] - rp[(size_t)i]); }
  }
  if (!longs_unsorted.empty()) {
    uint64_t *k0 = nullptr, *k1 = nullptr;
    V *v0 = nullptr, *v1 = nullptr;
    sc.take(&k0, (size_t)longest); sc.take(&k1, (size_t)longest); sc.take(&v0, (size_t)longest); sc.take(&v1, (size_t)longest);
    if (sc.oom) { *why = no_memory(std::string("sorting a ") + w.row + " of " + std::to_string(longest) + " " + w.items); return 1; }
    for (int64_t i : longs_unsorted)
      launch_csr_build_sort_long(st, rp[(size_t)i], rp[(size_t)i + 1] - rp[(size_t)i], ocol, oval, tie, k0, v0, k1, v1);
  }
  return 0;
}

// a valid pattern: the previous operator goes, and the canonical offsets of this rank (s.rp, and rp on the host) are built in its place
int pattern_begin_dev(const Entry& en, BuildScratch& sc, DevPattern& P, std::vector<int64_t>& rp, std::string* why) {
  if (int rc = pattern_validate_dev(en.e, sc, P, en.w, why)) return rc;
  CHK(operator_goes(en.e, en.which, true));
  return pattern_offsets_dev(en.e, sc, P, en.w, &en.e->op[en.which].sp.rp, rp, why);
}

// (DAV_CSR_DIAGONALS) the marks of the caller's validated arrays on the device, read back: the list and the decision of the host entry
int dia_decide_dev(E* e, BuildScratch& sc, const DevPattern& P, std::vector<int32_t>& offs, std::string* why) {
  const size_t nmarks = P.n > 0 ? (size_t)(2 * P.n - 1) : 0;
  uint8_t* marks = nullptr;
  unsigned long long* ndiag = nullptr;
  sc.take(&marks, nmarks); sc.take(&ndiag, 1);
  if (sc.oom) { *why = no_memory("the marks of " + std::to_string(nmarks) + " offsets"); return 1; }
  HIPCHK(hipMemsetAsync(marks, 0, std::max<size_t>(nmarks, 1), e->stream));
  HIPCHK(hipMemsetAsync(ndiag, 0, sizeof(unsigned long long), e->stream));
  launch_dia_mark(e->stream, P.row_ptr, P.rp64, P.col_idx, P.ci64, P.n, P.nnz, P.base, P.lower ? 1 : 0, marks, ndiag);
  std::vector<uint8_t> hmarks(std::max<size_t>(nmarks, 1));
  unsigned long long hdiag = 0;
  CHK(readback(e->stream, hmarks.data(), marks, nmarks));
  CHK(readback(e->stream, &hdiag, ndiag, sizeof(hdiag)));
  return dia_decide(hmarks.data(), P.n, P.nnz, (int64_t)hdiag, P.lower, offs, why) ? 0 : 1;
}

// the diagonal of the whole matrix on the device
double* diag_scratch(BuildScratch& sc, int64_t n, std::string* why) {
  double* d = nullptr;
  sc.take(&d, (size_t)n);
  if (sc.oom) *why = no_memory("the diagonal");
  return d;
}

// (dav_keep_value_map) the diagonal sources of the whole matrix from the counts and first positions of the check pass - the offsets by a
// scan of the counts, then one thread per row (block row) writes its positions - and the description of the caller's vals
int keep_diag_sources(const Entry& en, BuildScratch& sc, const DevPattern& P, int triangle, int rowmaj, std::string* why) {
  E* e = en.e;
  SparseStore& s = e->op[en.which].sp;
  int64_t* tile_sums = nullptr;
  sc.take(&tile_sums, (size_t)csr_build_scan_tiles(P.n));
  if (sc.oom || !keep(&s.doff, (size_t)P.n + 1)) { *why = map_memory(en.w); return 1; }
  launch_sparse_build_diag_counts(e->stream, P.dcount, P.n, s.doff);
  launch_csr_build_scan(e->stream, s.doff + 1, P.n, tile_sums);
  int64_t total = 0;
  CHK(readback(e->stream, &total, s.doff + P.n, sizeof(total)));
  if (!keep(&s.dpos, (size_t)total)) { *why = map_memory(en.w); return 1; }
  launch_sparse_build_diag_sources(e->stream, P.row_ptr, P.rp64, P.col_idx, P.ci64, P.n, P.base, P.dcount, P.dfirst, s.doff, s.dpos);
  s.gcount = P.nnz;
  s.triangle = triangle;
  s.rowmaj = rowmaj;
  return 0;
}
}  // namespace

// Validation, canonical rows, diagonal and storage equal those of dav_set_operator_csr bit for bit; only the work list is built on the
// host, over the canonical row offsets read back (8 (nloc + 1) bytes).
extern "C" int dav_set_operator_csr_dev(dav_handle_t e, int which, const void* row_ptr, int row_ptr_bits, const void* col_idx, int col_bits,
                                        const double* vals, int index_base, int triangle) {
  CHK(entry_begin(e, which, "dav_set_operator_csr_dev"));
  const Entry en{e, which, "dav_set_operator_csr_dev", CSR_WORDS};
  const int bits[2] = {row_ptr_bits, col_bits};
  std::string why = bad_arguments(en.w, e->n, false, 0, index_base, triangle, 0, bits, row_ptr);
  if (!why.empty()) return en.refuse(why);
  BuildScratch sc(e->stream);
  DevPattern P{row_ptr, row_ptr_bits == 64, col_idx, col_bits == 64, vals, 8, e->n, e->row0, e->nloc, index_base, (triangle & DAV_CSR_LOWER) != 0};
  std::vector<int64_t> rp;
  if (int rc = pattern_begin_dev(en, sc, P, rp, &why)) return en.step(rc, why);
  std::vector<int32_t> dia_offsets;
  if (triangle & DAV_CSR_DIAGONALS)
    if (int rc = dia_decide_dev(e, sc, P, dia_offsets, &why)) return en.step(rc, why);
  SparseStore& s = e->op[which].sp;
  const int64_t lnnz = rp.back();
  if (!keep(&s.col, (size_t)lnnz) || !keep(&s.val, (size_t)lnnz)) return en.refuse(no_memory(stored(en.w, lnnz, 12 * lnnz + 8 * e->nloc)));
  const bool keep_map = e->keep_map[which] != 0;
  if (keep_map) {          // the order with the source of an entry as payload (as BSR has it); the values then follow their sources
    if (!keep(&s.src, (size_t)lnnz)) return en.refuse(map_memory(en.w));
    if (int rc = pattern_order_dev(e, sc, P, en.w, s.rp, rp, s.col, s.src, &why)) return en.step(rc, why);
    launch_sparse_refresh_csr(e->stream, s.src, lnnz, vals, s.val);
  } else {
    if (int rc = pattern_order_dev(e, sc, P, en.w, s.rp, rp, s.col, s.val, &why)) return en.step(rc, why);
  }
  double* diag = diag_scratch(sc, e->n, &why);
  if (!diag) return en.refuse(why);
  launch_csr_build_diag(e->stream, row_ptr, P.rp64, col_idx, P.ci64, vals, e->n, index_base, P.dcount, P.dfirst, diag);
  if (keep_map)
    if (int rc = keep_diag_sources(en, sc, P, triangle & DAV_CSR_LOWER, 0, &why)) return en.step(rc, why);
  std::vector<double> hdiag;
  CHK(sparse_commit(en, DAV_KIND_CSR, 1, 0, rp, hdiag, diag, no_memory(work_list(en.w, lnnz))));
  return (triangle & DAV_CSR_DIAGONALS) ? dia_commit(en, dia_offsets) : 0;
}

// COO triples in device memory (kernels in k_coo_build.hip).  Everything is validated in scratch before the previous
// operator goes and anything is allocated for the new one.  Scratch (BuildScratch, released before return): 8 (nloc + 1) + 8 nloc bytes
// for the counts and slot cursors of this rank's rows, 16 (n + 1) + 8 n for those of the diagonal pattern and the diagonal, 4 bytes per
// canonical entry of this rank (the tie) and 16 per diagonal entry of the matrix (12 when the value map keeps their positions), nloc + n
// bytes of row flags where a row is longer than 64 entries, 2 n - 1 bytes of marks with DAV_CSR_DIAGONALS, and 32 bytes per entry of the
// longest row above 2048 entries.
extern "C" int davx_set_operator_coo_dev(dav_handle_t e, int which, int64_t nnz, const void* row_idx, int row_bits, const void* col_idx,
                                        int col_bits, const double* vals, int index_base, int triangle) {
  CHK(entry_begin(e, which, "davx_set_operator_coo_dev"));
  const Entry en{e, which, "davx_set_operator_coo_dev", COO_WORDS};
  const int bits[2] = {row_bits, col_bits};
  const int64_t n = e->n, nloc = e->nloc, r0 = e->row0;
  std::string why = bad_triples(n, nnz, index_base, triangle, bits, row_idx, col_idx, vals);
  if (!why.empty()) return en.refuse(why);
  const int ri64 = row_bits == 64, ci64 = col_bits == 64, lower = (triangle & DAV_CSR_LOWER) ? 1 : 0;
  if (nnz > 0 && (!device_array(e, row_idx, en.w.rp, (ri64 ? 8 : 4) * (size_t)nnz, &why) ||
                  !device_array(e, col_idx, en.w.ci, (ci64 ? 8 : 4) * (size_t)nnz, &why) || !device_array(e, vals, "vals", 8 * (size_t)nnz, &why)))
    return en.refuse(why);
  hipStream_t st = e->stream;
  BuildScratch sc(st);
  // check / count: the first offending triple; the lengths of this rank's canonical rows and of the rows of the diagonal pattern
  unsigned long long *info = nullptr, *lcount = nullptr, *dcount = nullptr;
  int64_t *locate = nullptr, *tile_sums = nullptr;
  sc.take(&info, 1); sc.take(&locate, 2); sc.take(&lcount, (size_t)nloc + 1); sc.take(&dcount, (size_t)n + 1);
  sc.take(&tile_sums, (size_t)csr_build_scan_tiles(n));
  if (sc.oom) return en.refuse(no_memory("the validation of " + std::to_string(n) + " " + en.w.rows));
  HIPCHK(hipMemsetAsync(info, 0xff, sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(lcount, 0, sizeof(unsigned long long) * ((size_t)nloc + 1), st));
  HIPCHK(hipMemsetAsync(dcount, 0, sizeof(unsigned long long) * ((size_t)n + 1), st));
  launch_coo_build_check(st, row_idx, ri64, col_idx, ci64, n, nnz, index_base, lower, r0, nloc, info, lcount + 1, dcount + 1);
  unsigned long long first_bad = 0;
  CHK(readback(st, &first_bad, info, sizeof(first_bad)));
  if (first_bad != ~0ull) {
    launch_coo_build_locate(st, row_idx, ri64, col_idx, ci64, (int64_t)first_bad, locate);
    int64_t loc[2];
    CHK(readback(st, loc, locate, sizeof(loc)));
    return en.refuse(msg_bad_triple(en.w, n, index_base, (int64_t)first_bad, loc[0], loc[1]));
  }
  std::vector<int32_t> dia_offsets;
  if (triangle & DAV_CSR_DIAGONALS) {          // the marks of the validated triples, read back: the list and the decision of the host entry
    const size_t nmarks = (size_t)(2 * n - 1);
    uint8_t* marks = nullptr;
    unsigned long long* ndiag = nullptr;
    sc.take(&marks, nmarks); sc.take(&ndiag, 1);
    if (sc.oom) return en.refuse(no_memory("the marks of " + std::to_string(nmarks) + " offsets"));
    HIPCHK(hipMemsetAsync(marks, 0, nmarks, st));
    HIPCHK(hipMemsetAsync(ndiag, 0, sizeof(unsigned long long), st));
    launch_coo_mark(st, row_idx, ri64, col_idx, ci64, n, nnz, index_base, lower, marks, ndiag);
    std::vector<uint8_t> hmarks(nmarks);
    unsigned long long hdiag = 0;
    CHK(readback(st, hmarks.data(), marks, nmarks));
    CHK(readback(st, &hdiag, ndiag, sizeof(hdiag)));
    if (!dia_decide(hmarks.data(), n, nnz, (int64_t)hdiag, lower != 0, dia_offsets, &why)) return en.refuse(why);
  }
  // offsets: the two count arrays scanned in place (a leading 0 each); those of this rank's rows stay with the operator
  CHK(operator_goes(e, which, true));
  SparseStore& s = e->op[which].sp;
  int64_t* lrp = (int64_t*)lcount;
  int64_t* doff = (int64_t*)dcount;
  launch_csr_build_scan(st, lrp + 1, nloc, tile_sums);
  launch_csr_build_scan(st, doff + 1, n, tile_sums);
  std::vector<int64_t> rp((size_t)nloc + 1), hdoff((size_t)n + 1);
  CHK(readback(st, rp.data(), lrp, sizeof(int64_t) * rp.size()));
  CHK(readback(st, hdoff.data(), doff, sizeof(int64_t) * hdoff.size()));
  const int64_t lnnz = rp.back(), ndiag = hdoff.back();
  const bool keep_map = e->keep_map[which] != 0;
  if (!keep(&s.rp, (size_t)nloc + 1) || !keep(&s.col, (size_t)lnnz) || !keep(&s.val, (size_t)lnnz))
    return en.refuse(no_memory(stored(en.w, lnnz, 12 * lnnz + 8 * nloc)));
  if (keep_map && (!keep(&s.src, (size_t)lnnz) || !keep(&s.doff, (size_t)n + 1) || !keep(&s.dpos, (size_t)ndiag))) return en.refuse(map_memory(en.w));
  HIPCHK(hipMemcpyAsync(s.rp, lrp, sizeof(int64_t) * ((size_t)nloc + 1), hipMemcpyDeviceToDevice, st));
  // scatter: atomic slots (the cursors start at the offsets), then the sorts remove the slot order
  unsigned long long *cursor = nullptr, *dcursor = nullptr;
  uint32_t *tie = nullptr, *dtie = nullptr;
  int32_t* dcol = nullptr;
  uint64_t* dpos = (uint64_t*)s.dpos;
  double* diag = nullptr;
  sc.take(&cursor, (size_t)nloc); sc.take(&dcursor, (size_t)n); sc.take(&tie, (size_t)lnnz); sc.take(&dtie, (size_t)ndiag);
  sc.take(&dcol, (size_t)ndiag); sc.take(&diag, (size_t)n);
  if (!keep_map) sc.take(&dpos, (size_t)ndiag);
  if (sc.oom) return en.refuse(no_memory("sorting " + std::to_string(lnnz) + " " + en.w.items));
  if (nloc > 0) HIPCHK(hipMemcpyAsync(cursor, lrp, sizeof(int64_t) * (size_t)nloc, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(dcursor, doff, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemsetAsync(dcol, 0, sizeof(int32_t) * std::max<size_t>((size_t)ndiag, 1), st));
  if (keep_map) launch_coo_build_scatter(st, row_idx, ri64, col_idx, ci64, vals, nnz, index_base, lower, r0, nloc, cursor, s.col, s.src, tie, dcursor, dtie, dpos);
  else launch_coo_build_scatter(st, row_idx, ri64, col_idx, ci64, vals, nnz, index_base, lower, r0, nloc, cursor, s.col, s.val, tie, dcursor, dtie, dpos);
  // sort: rows of at most 64 entries in registers; only where longer rows exist, the flag pass and the LDS / tile-and-merge sorts
  auto order = [&](const int64_t* offs, const std::vector<int64_t>& hoffs, int32_t* ocol, auto* oval, uint32_t* t) -> int {
    const int64_t nrows = (int64_t)hoffs.size() - 1;
    launch_coo_sort_small(st, offs, nrows, ocol, oval, t);
    bool longer = false;
    for (int64_t i = 0; i < nrows && !longer; ++i) longer = hoffs[(size_t)i + 1] - hoffs[(size_t)i] > coo_sort_small_rows();
    if (!longer) return 0;
    uint8_t* flag = nullptr;
    sc.take(&flag, (size_t)nrows);
    if (sc.oom) { why = no_memory("sorting " + std::to_string(hoffs.back()) + " " + en.w.items); return 1; }
    return pattern_sort_dev(e, sc, en.w, offs, hoffs, ocol, oval, t, flag, &why);
  };
  if (int rc = keep_map ? order(s.rp, rp, s.col, s.src, tie) : order(s.rp, rp, s.col, s.val, tie)) return en.step(rc, why);
  if (int rc = order(doff, hdoff, dcol, dpos, dtie)) return en.step(rc, why);
  if (keep_map) {          // the values follow their sources; the sorted diagonal pattern is the diagonal sources
    launch_sparse_refresh_csr(st, s.src, lnnz, vals, s.val);
    HIPCHK(hipMemcpyAsync(s.doff, doff, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToDevice, st));
    s.gcount = nnz;
    s.triangle = triangle & DAV_CSR_LOWER;
    s.rowmaj = 0;
  }
  // the diagonal of the whole matrix: per row from +0.0 in ascending p
  launch_sparse_refresh_diag(st, 1, doff, (const int64_t*)dpos, vals, n, diag);
  std::vector<double> hdiag;
  CHK(sparse_commit(en, DAV_KIND_CSR, 1, 0, rp, hdiag, diag, no_memory(work_list(en.w, lnnz))));
  return (triangle & DAV_CSR_DIAGONALS) ? dia_commit(en, dia_offsets) : 0;
}

// The index level is the CSR device build over the n / b block rows, local block rows = those that touch the slab, with the SOURCE of a
// block (input position, mirrored or not) as payload; the values then move once (launch_bsr_build_gather).  Validation, canonical block
// rows, values, diagonal and work list equal those of dav_set_operator_bsr bit for bit.
// pairs (davh_set_operator_csr_dev): vals holds one (re, im) pair per block, b = 2; the 16 bytes of an entry are read where they lie -
// by the diagonal pass, which runs right after the pattern is validated, before anything is allocated for the new operator (a refusal
// releases the previous operator, as every refusal of a set entry does), and by the gather.
namespace {
int set_bsr_dev(const Entry& en, int b, const void* block_row_ptr, int row_ptr_bits, const void* block_col_idx, int col_bits, const double* vals,
                int index_base, int triangle, int block_layout, bool pairs) {
  E* e = en.e;
  const int which = en.which;
  const int64_t n = e->n;
  std::string why;
  const int64_t nb = n / b, bb = (int64_t)b * b;
  int64_t ib0, nbl;
  local_block_rows(e, b, &ib0, &nbl);
  BuildScratch sc(e->stream);
  DevPattern P{block_row_ptr, row_ptr_bits == 64, block_col_idx, col_bits == 64, vals, pairs ? 16 : 8 * (size_t)bb, nb, ib0, nbl, index_base,
               triangle == DAV_CSR_LOWER};
  std::vector<int64_t> rp;
  double* diag = nullptr;
  if (pairs) {
    if (((uintptr_t)vals & 15) != 0) return en.refuse("vals is not aligned to 16 bytes (one complex value)");
    if (int rc = pattern_validate_dev(e, sc, P, en.w, &why)) return en.step(rc, why);
    unsigned long long* bad = nullptr;
    sc.take(&bad, 1);
    diag = diag_scratch(sc, n, &why);
    if (!diag) return en.refuse(why);
    HIPCHK(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), e->stream));
    launch_bsr_build_diag_pairs(e->stream, block_row_ptr, P.rp64, block_col_idx, P.ci64, vals, nb, index_base, P.dcount, P.dfirst, diag, bad);
    unsigned long long first_bad = 0;
    CHK(readback(e->stream, &first_bad, bad, sizeof(first_bad)));
    if (first_bad != ~0ull) {          // the diagonal entry p lies in row col_idx[p]
      int64_t* locate = nullptr;
      sc.take(&locate, 2);
      if (sc.oom) return en.refuse(no_memory("the validation"));
      launch_csr_build_locate(e->stream, P.row_ptr, P.rp64, P.col_idx, P.ci64, nb, P.base, (int64_t)first_bad, locate);
      int64_t loc[2];
      double im = 0.0;
      CHK(readback(e->stream, loc, locate, sizeof(loc)));
      CHK(readback(e->stream, &im, vals + 2 * (int64_t)first_bad + 1, sizeof(im)));
      return en.refuse(msg_imag_diagonal(en.w, index_base, (int64_t)first_bad, loc[0], im));
    }
    CHK(operator_goes(e, which, true));
    if (int rc = pattern_offsets_dev(e, sc, P, en.w, &e->op[which].sp.rp, rp, &why)) return en.step(rc, why);
  } else if (int rc = pattern_begin_dev(en, sc, P, rp, &why)) {
    return en.step(rc, why);
  }
  SparseStore& s = e->op[which].sp;
  const int64_t lnnzb = rp.back();
  const bool keep_map = e->keep_map[which] != 0;
  uint64_t* src = nullptr;          // source of each canonical block: input block p << 1 | mirrored (dav_keep_value_map: stays with the operator)
  if (!keep_map) sc.take(&src, (size_t)lnnzb);
  else if (keep(&s.src, (size_t)lnnzb)) src = s.src;
  if (!src || sc.oom || !keep(&s.col, (size_t)lnnzb) || !keep(&s.val, (size_t)(lnnzb * bb)))
    return en.refuse(no_memory(stored(en.w, lnnzb, lnnzb * (8 * bb + 12))));
  if (int rc = pattern_order_dev(e, sc, P, en.w, s.rp, rp, s.col, src, &why)) return en.step(rc, why);
  // the values: column-major per block, a mirrored block the transpose of its source
  if (pairs) {
    launch_bsr_build_gather_pairs(e->stream, src, lnnzb, vals, s.val);
  } else {
    launch_bsr_build_gather(e->stream, b, src, lnnzb, vals, block_layout == DAV_BSR_ROW_MAJOR ? 1 : 0, s.val);
    diag = diag_scratch(sc, n, &why);
    if (!diag) return en.refuse(why);
    launch_bsr_build_diag(e->stream, b, block_row_ptr, P.rp64, block_col_idx, P.ci64, vals, nb, index_base, P.dcount, P.dfirst, diag);
  }
  if (keep_map) {
    if (int rc = keep_diag_sources(en, sc, P, triangle, block_layout == DAV_BSR_ROW_MAJOR ? 1 : 0, &why)) return en.step(rc, why);
    s.pairs = pairs ? 1 : 0;
    s.pairs_base = index_base;
  }
  std::vector<double> hdiag;
  return sparse_commit(en, DAV_KIND_BSR, b, ib0 * b - e->row0, rp, hdiag, diag, no_memory(work_list(en.w, lnnzb)));
}
}  // namespace

extern "C" int dav_set_operator_bsr_dev(dav_handle_t e, int which, int block_size, const void* block_row_ptr, int row_ptr_bits,
                                        const void* block_col_idx, int col_bits, const double* vals, int index_base, int triangle,
                                        int block_layout) {
  CHK(entry_begin(e, which, "dav_set_operator_bsr_dev"));
  const Entry en{e, which, "dav_set_operator_bsr_dev", BSR_WORDS};
  const int bits[2] = {row_ptr_bits, col_bits};
  const std::string why = bad_arguments(en.w, e->n, true, block_size, index_base, triangle, block_layout, bits, block_row_ptr);
  if (!why.empty()) return en.refuse(why);
  return set_bsr_dev(en, block_size, block_row_ptr, row_ptr_bits, block_col_idx, col_bits, vals, index_base, triangle, block_layout, false);
}

// A complex Hermitian CSR matrix of order n / 2 in device arrays: the device BSR build with b = 2 over the caller's pattern, reading pairs.
// No scratch holds expanded values.
extern "C" int davh_set_operator_csr_dev(dav_handle_t e, int which, const void* row_ptr, int row_ptr_bits, const void* col_idx, int col_bits,
                                         const double* vals, int index_base, int triangle) {
  CHK(entry_begin(e, which, "davh_set_operator_csr_dev"));
  const Entry en{e, which, "davh_set_operator_csr_dev", CSR_WORDS};
  const int bits[2] = {row_ptr_bits, col_bits};
  const std::string why = bad_arguments_herm(en.w, e->n, index_base, triangle, bits, row_ptr);
  if (!why.empty()) return en.refuse(why);
  return set_bsr_dev(en, 2, row_ptr, row_ptr_bits, col_idx, col_bits, vals, index_base, triangle, DAV_BSR_ROW_MAJOR, true);
}

// ---- new values on the kept pattern ------------------------------------------------------------------------------------------------------
// The fifth entry of the shared structure: steps 3 (values) and 4 (diagonal) alone, over what a set call made with dav_keep_value_map on
// left with the operator.  rp, col, the work list, the partial slots and the maps are read or left alone, never written.
extern "C" int dav_keep_value_map(dav_handle_t e, int which, int on) {
  if (!e) return fail("dav_keep_value_map: null engine");
  if (which < 0 || which >= N_OPS) return fail("dav_keep_value_map: bad operator id");
  if (on != 0 && (e->op[which].kind == DAV_KIND_FSAI || e->op[which].kind == DAV_KIND_BFSAI))
    return fail(std::string("dav_keep_value_map: the operator is ") + kind_words(e->op[which].kind) + ": it has no value map to keep");
  e->keep_map[which] = on != 0 ? 1 : 0;
  return 0;
}

namespace {
// a refused update leaves the operator as it is: set, with its old values
int update_refuse(const char* name, const std::string& msg) { return fail(std::string(name) + ": " + msg); }

// "" = the operator can take new values: CSR (also stored by diagonals) or BSR, set with its value map
std::string not_updatable(const OpDesc& o) {
  if (o.kind == DAV_KIND_NONE) return "operator not set";
  if (o.kind == DAV_KIND_FSAI) return std::string("the operator is ") + kind_words(o.kind) + ": a snapshot of A, B and sigma that takes no values (call davp_build_fsai again)";
  if (o.kind == DAV_KIND_BFSAI) return std::string("the operator is ") + kind_words(o.kind) + ": a snapshot of A, B and sigma that takes no values (call davq_build_block_fsai again)";
  if (o.kind != DAV_KIND_CSR && o.kind != DAV_KIND_BSR && o.kind != DAV_KIND_DIA)
    return "the operator is not a CSR or BSR operator (only a sparse operator set after dav_keep_value_map(h, which, 1) takes new values)";
  if (!o.sp.src || !o.sp.doff || !o.sp.dpos)
    return "the operator was set without its value map: call dav_keep_value_map(h, which, 1) before the set call";
  return "";
}

// vals: the caller's values in device memory, as long as the set call's
int update_from_device(E* e, int which, const char* name, BuildScratch& sc, const double* vals) {
  OpDesc& o = e->op[which];
  const SparseStore& s = o.sp;
  hipStream_t st = e->stream;
  double* diag = nullptr;          // the diagonal of the whole matrix (o.diag holds the local rows)
  sc.take(&diag, (size_t)e->n);
  if (sc.oom) return update_refuse(name, no_memory("the diagonal"));
  if (s.pairs) {          // (re, im) pairs: the diagonal first - an imaginary diagonal is refused before a value moves
    unsigned long long* bad = nullptr;
    sc.take(&bad, 1);
    if (sc.oom) return update_refuse(name, no_memory("the diagonal"));
    HIPCHK(hipMemsetAsync(bad, 0xff, sizeof(unsigned long long), st));
    launch_bsr_refresh_diag_pairs(st, s.doff, s.dpos, vals, e->n / 2, diag, bad);
    unsigned long long first_bad = 0;
    CHK(readback(st, &first_bad, bad, sizeof(first_bad)));
    if (first_bad != ~0ull) {          // the text of the set entries: the row of entry p from the kept diagonal sources (ascending in p)
      const int64_t nb = e->n / 2, p = (int64_t)first_bad;
      std::vector<int64_t> doff((size_t)nb + 1);
      CHK(readback(st, doff.data(), s.doff, sizeof(int64_t) * doff.size()));
      std::vector<int64_t> dpos((size_t)doff.back());
      CHK(readback(st, dpos.data(), s.dpos, sizeof(int64_t) * dpos.size()));
      const int64_t t = std::lower_bound(dpos.begin(), dpos.end(), p) - dpos.begin();
      const int64_t row = std::upper_bound(doff.begin(), doff.end(), t) - doff.begin() - 1;
      double im = 0.0;
      CHK(readback(st, &im, vals + 2 * p + 1, sizeof(im)));
      return update_refuse(name, msg_imag_diagonal(CSR_WORDS, s.pairs_base, p, row, im));
    }
    launch_bsr_build_gather_pairs(st, s.src, s.nnz, vals, s.val);
  } else if (o.kind == DAV_KIND_BSR) launch_bsr_build_gather(st, s.b, s.src, s.nnz, vals, s.rowmaj, s.val);
  else launch_sparse_refresh_csr(st, s.src, s.nnz, vals, s.val);
  if (o.kind == DAV_KIND_DIA) dia_fill(e, s);        // the slots follow the values, as the set call filled them
  o.sp.bdiag_valid = false;          // the diagonal blocks of a BDPR correction follow the values: rebuilt at the next one
  o.sp.rbound_valid = false;         // ... and the row-sum bound of a CHEB correction
  o.lbound_valid = false;            // ... and the Lanczos bound of an LCHEB correction
  if (!s.pairs) launch_sparse_refresh_diag(st, s.b, s.doff, s.dpos, vals, e->n, diag);
  if (e->nloc > 0) HIPCHK(hipMemcpyAsync(o.diag, diag + e->row0, sizeof(double) * e->nloc, hipMemcpyDeviceToDevice, st));
  // what depends on the numbers: the diagonal on the host and the start-vector order of A
  if (which == DAV_OP_A) e->basis_order.clear();
  e->diag_host[which].resize((size_t)e->n);
  return readback(st, e->diag_host[which].data(), diag, sizeof(double) * (size_t)e->n);     // ends synchronised: vals is free again
}
}  // namespace

extern "C" int dav_update_operator_values(dav_handle_t e, int which, const double* vals) {
  const char* name = "dav_update_operator_values";
  CHK(entry_begin(e, which, name));
  const std::string why = not_updatable(e->op[which]);
  if (!why.empty()) return update_refuse(name, why);
  const SparseStore& s = e->op[which].sp;
  const size_t count = (size_t)s.gcount * (s.pairs ? 2 : (size_t)s.b * (size_t)s.b);
  if (count > 0 && !vals) return update_refuse(name, "null vals");
  BuildScratch sc(e->stream);
  double* dvals = nullptr;
  sc.take(&dvals, count);
  if (sc.oom) return update_refuse(name, no_memory("the " + std::to_string(count) + " values"));
  if (count > 0) HIPCHK(hipMemcpyAsync(dvals, vals, sizeof(double) * count, hipMemcpyHostToDevice, e->stream));
  return update_from_device(e, which, name, sc, dvals);
}

extern "C" int dav_update_operator_values_dev(dav_handle_t e, int which, const double* vals_dev) {
  const char* name = "dav_update_operator_values_dev";
  CHK(entry_begin(e, which, name));
  std::string why = not_updatable(e->op[which]);
  if (!why.empty()) return update_refuse(name, why);
  const SparseStore& s = e->op[which].sp;
  const size_t count = (size_t)s.gcount * (s.pairs ? 2 : (size_t)s.b * (size_t)s.b);
  if (count > 0) {
    if (!vals_dev) return update_refuse(name, "null vals");
    if (!device_array(e, vals_dev, "vals", sizeof(double) * count, &why)) return update_refuse(name, why);
    if (s.pairs && ((uintptr_t)vals_dev & 15) != 0) return update_refuse(name, "vals is not aligned to 16 bytes (one complex value)");
  }
  BuildScratch sc(e->stream);
  return update_from_device(e, which, name, sc, vals_dev);
}
