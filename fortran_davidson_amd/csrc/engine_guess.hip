// Engine, warm start: a solve that begins from vectors the caller has - or from the Ritz vectors the last solve left - instead of the
// unit vectors of dav_init_basis.  One mechanism: a staged guess is X columns [0, guess_cols) (engine_internal.h); dav_set_guess /
// dav_set_guess_dev put a caller's array there through guess_ingest_kernel (k_guess.hip), dav_mark_result_as_guess records that a
// driver's Ritz vectors already lie there, dav_init_basis_guess moves the staged columns to the front of the basis.  Everything
// after that - orthonormalisation, the first sweep (dav_expand), the projection - is the code every later iteration runs.
#include "engine_internal.h"

namespace {
int guess_refuse(const char* name, const std::string& msg) { return fail(std::string(name) + ": " + msg); }

// the scalar rules of both set entries ("" = fine)
std::string guess_bad_shape(const E* e, const void* x, int64_t ldx, int ncols) {
  if (ncols < 1) return "ncols = " + std::to_string(ncols) + " must be at least 1";
  if (ncols > e->max_cols) return "ncols = " + std::to_string(ncols) + " exceeds the engine's max_cols = " + std::to_string(e->max_cols);
  if (ldx < e->n) return "ldx = " + std::to_string(ldx) + " is smaller than n = " + std::to_string(e->n);
  if (!x) return "x is a null pointer";
  return "";
}

// What the ingest passes found, made common over the ranks (every rank refuses or accepts together), and the verdict: the columns land
// in the scratch panel first because the answer is only known after the pass and a refused call must leave X - and with it a guess
// staged earlier - as it was; an accepted guess then moves to X on the device.
int guess_commit(E* e, const char* name, int ncols) {
  const int words = guess_flag_words(ncols);
  std::vector<unsigned long long> fl((size_t)words);
  HIPCHK(hipMemcpyAsync(fl.data(), e->guess_flags, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  std::vector<double> seen((size_t)ncols + 1);
  seen[0] = (fl[0] & 1ull) ? 1.0 : 0.0;
  for (int c = 0; c < ncols; ++c) seen[(size_t)c + 1] = ((fl[1 + c / 64] >> (c % 64)) & 1ull) ? 1.0 : 0.0;
  if (e->nranks > 1) {
    CHK(need_comm(e));
    HIPCHK(hipMemcpyAsync(e->gram_dev, seen.data(), sizeof(double) * seen.size(), hipMemcpyHostToDevice, e->stream));
    CHK(coll_allreduce(e, e->gram_dev, seen.size()));
    HIPCHK(hipMemcpyAsync(seen.data(), e->gram_dev, sizeof(double) * seen.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if (seen[0] != 0.0) return guess_refuse(name, "x holds an entry that is not finite (Inf or NaN)");
  for (int c = 0; c < ncols; ++c)
    if (seen[(size_t)c + 1] == 0.0) return guess_refuse(name, "column " + std::to_string(c) + " of x (counted from 0) is entirely zero");
  launch_copy_columns(e->stream, panel_ptr(e, DAV_PANEL_S, 0), e->ldp, panel_ptr(e, DAV_PANEL_X, 0), e->ldp, e->nloc_pad, ncols);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  e->guess_cols = ncols;
  e->guess_tag = GUESS_ONE_SHOT;
  return 0;
}

int guess_staged(const E* e) {
  if (e->guess_tag == GUESS_ONE_SHOT) return e->guess_cols;
  if (e->guess_tag == GUESS_RESULT && e->keep_result) return e->guess_cols;
  return 0;
}
}  // namespace

extern "C" int dav_set_guess(dav_handle_t e, const double* x, int64_t ldx, int ncols) {
  const char* name = "dav_set_guess";
  if (!e) return fail(std::string(name) + ": null engine");
  CHK(bind(e));
  const std::string why = guess_bad_shape(e, x, ldx, ncols);
  if (!why.empty()) return guess_refuse(name, why);
  hipStream_t st = e->stream;
  double* S = panel_ptr(e, DAV_PANEL_S, 0);
  HIPCHK(hipMemsetAsync(e->guess_flags, 0, sizeof(unsigned long long) * guess_flag_words(ncols), st));
  // this rank's rows of the global array, in row blocks through two of the engine's pinned small buffers and their device twins
  // (column-major blocks of `take` rows), each block by the kernel of the device entry; an even block height keeps the 16-byte lanes
  const int64_t cap = (int64_t)(e->small_doubles / (size_t)ncols) / 2 * 2;
  if (cap < 2) return guess_refuse(name, "the engine's staging buffers are too small for " + std::to_string(ncols) + " columns");
  const int64_t pad = e->nloc_pad - e->nloc;
  if (e->nloc == 0 && pad > 0) launch_guess_ingest(st, S, e->ldp, 0, ncols, pad, S, e->ldp, e->guess_flags);     // a rank without rows: zeros
  int flip = 0;
  for (int64_t r = 0; r < e->nloc; r += cap, flip ^= 1) {
    const int64_t take = std::min(cap, e->nloc - r);
    SmallBuf& b = e->sm[2 + flip];
    if (b.pending) { HIPCHK(hipEventSynchronize(b.done)); b.pending = false; }
    for (int c = 0; c < ncols; ++c)
      std::memcpy(b.host + (size_t)c * take, x + (int64_t)c * ldx + e->row0 + r, sizeof(double) * (size_t)take);
    HIPCHK(hipMemcpyAsync(b.dev, b.host, sizeof(double) * (size_t)take * ncols, hipMemcpyHostToDevice, st));
    launch_guess_ingest(st, b.dev, take, take, ncols, r + take == e->nloc ? pad : 0, S + r, e->ldp, e->guess_flags);
    HIPCHK(hipEventRecord(b.done, st));
    b.pending = true;
  }
  HIPCHK(hipGetLastError());
  return guess_commit(e, name, ncols);
}

extern "C" int dav_set_guess_dev(dav_handle_t e, const double* x_dev, int64_t ldx, int ncols) {
  const char* name = "dav_set_guess_dev";
  if (!e) return fail(std::string(name) + ": null engine");
  CHK(bind(e));
  std::string why = guess_bad_shape(e, x_dev, ldx, ncols);
  if (!why.empty()) return guess_refuse(name, why);
  if (!device_array(e, x_dev, "x_dev", sizeof(double) * (size_t)(ldx * (int64_t)(ncols - 1) + e->n), &why)) return guess_refuse(name, why);
  HIPCHK(hipMemsetAsync(e->guess_flags, 0, sizeof(unsigned long long) * guess_flag_words(ncols), e->stream));
  double* S = panel_ptr(e, DAV_PANEL_S, 0);
  // (a rank without rows reads nothing: nrows = 0, its pad rows are zeroed)
  launch_guess_ingest(e->stream, x_dev + (e->nloc > 0 ? e->row0 : 0), ldx, e->nloc, ncols, e->nloc_pad - e->nloc, S, e->ldp, e->guess_flags);
  HIPCHK(hipGetLastError());
  return guess_commit(e, name, ncols);        // ends synchronised with the engine's stream: x_dev is free again
}

extern "C" int dav_keep_result_as_guess(dav_handle_t e, int on) {
  if (!e) return fail("dav_keep_result_as_guess: null engine");
  e->keep_result = on != 0 ? 1 : 0;
  return 0;
}

extern "C" int dav_mark_result_as_guess(dav_handle_t e, int ncols) {
  if (!e) return fail("dav_mark_result_as_guess: null engine");
  if (ncols < 0 || ncols > e->max_cols) return fail("dav_mark_result_as_guess: bad column count");
  e->guess_cols = ncols;
  e->guess_tag = ncols > 0 ? GUESS_RESULT : GUESS_NONE;
  return 0;
}

extern "C" int dav_guess_columns(dav_handle_t e, int* ncols) {
  if (!e || !ncols) return fail("dav_guess_columns: null argument");
  *ncols = guess_staged(e);
  return 0;
}

extern "C" int dav_init_basis_guess(dav_handle_t e, int ncols, int64_t* idx_out, int* nguess) {
  CHK(bind(e));                 // (drops what dav_init_basis may have left for the H0 shortcut: it only holds for pure unit columns)
  if (ncols <= 0 || ncols > e->max_cols || ncols > e->n) return fail("dav_init_basis_guess: bad column count");
  const int g = std::min(guess_staged(e), ncols);
  const int nfill = ncols - g;
  if (e->diag_host[DAV_OP_A].empty()) return fail("dav_init_basis_guess: operator A not set");
  basis_order_ensure(e, ncols);               // the order dav_init_basis takes its start vectors from: one cache, one rule
  if ((int)e->basis_order.size() < nfill) return fail("dav_init_basis_guess: bad column count");
  // the tickets of the last-workgroup finishes start every solve from zero, as in dav_init_basis
  HIPCHK(hipMemsetAsync(e->counters, 0, sizeof(unsigned) * (GRAM_MAX_COUNTERS + 8), e->stream));
  if (g > 0) launch_copy_columns(e->stream, panel_ptr(e, DAV_PANEL_X, 0), e->ldp, panel_ptr(e, DAV_PANEL_V, 0), e->ldp, e->nloc_pad, g);
  std::vector<int64_t> order(e->basis_order.begin(), e->basis_order.begin() + nfill);
  if (nfill > 0) {
    HIPCHK(hipMemcpyAsync(e->idx_dev, order.data(), sizeof(int64_t) * nfill, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    launch_unit_columns(e->stream, e->idx_dev, nfill, e->row0, e->nloc, e->nloc_pad, panel_ptr(e, DAV_PANEL_V, g), e->ldp);
  }
  HIPCHK(hipGetLastError());
  e->m = ncols;
  if (idx_out)
    for (int i = 0; i < ncols; ++i) idx_out[i] = i < g ? 0 : order[(size_t)(i - g)] + 1;
  if (nguess) *nguess = g;
  if (e->guess_tag == GUESS_ONE_SHOT) guess_drop(e);      // consumed; what a solve left stays offered until X is written again
  return 0;
}
