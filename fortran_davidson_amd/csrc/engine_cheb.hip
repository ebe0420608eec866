// Engine, the Chebyshev-filtered correction (DAV_METHOD_CHEB; include/davidson_hip.h states the recurrence and the interval): the contract
// of the method, the row-sum bound kept with a sparse operator, the workspace, and the step of the Ritz phase that turns the residues into
// the correction block by d - 1 block products (kernels in k_cheb.hip; the fused step of a CSR operator in k_spmm.hip).  Behind it the
// same correction for any operator the engine applies on the device (DAV_METHOD_LCHEB): its bound comes from a short Lanczos run with A
// (kernels in k_lanczos.hip) and is kept with operator A.
#include "engine_internal.h"

namespace {
// the refusals of both methods; the prefix says which
int refuse(int method, const std::string& why) { return fail((method == DAV_METHOD_LCHEB ? "LCHEB correction: " : "CHEB correction: ") + why); }
int ws_cols(const E* e) { return e->cols_alloc / 2 + 8; }     // the width of a block of the GJD workspace
size_t ws_block(const E* e) { return (size_t)e->ldp * ws_cols(e); }

// the workspace of the filter, shared by both methods: three column blocks, then the coefficients
int ensure_workspace(E* e, int method) {
  if (e->cheb_ws) return 0;
  const size_t bytes = sizeof(double) * (3 * ws_block(e) + cheb_coef_doubles(ws_cols(e)));
  if (pool_malloc(&e->cheb_ws, bytes) != hipSuccess) {
    (void)hipGetLastError();
    e->cheb_ws = nullptr;
    return refuse(method, "device memory for the workspace (" + std::to_string(bytes >> 20) + " MiB) could not be allocated");
  }
  HIPCHK(hipMemsetAsync(e->cheb_ws, 0, bytes, e->stream));
  return 0;
}

// ---- the Lanczos bound of DAV_METHOD_LCHEB ----------------------------------------------------------------------------------------------
// NaN-propagating maximum, as cheb_coef takes it
double nan_max(double m, double x) { return (x > m || x != x) ? x : m; }

// The dot product the last launch left in the slots: all-reduced, fetched, added in rank order (every slot but one is +0.0 before the
// all-reduce, so its sum is exact and every rank adds the same numbers in the same order)
int fetch_dot(E* e, double* slots, std::vector<double>& host, double* out) {
  if (has_comm(e)) CHK(coll_allreduce(e, slots, (size_t)e->nranks));
  HIPCHK(hipMemcpyAsync(host.data(), slots, sizeof(double) * (size_t)e->nranks, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  double s = host[0];
  for (int p = 1; p < e->nranks; ++p) s += host[p];
  *out = s;
  return 0;
}

// b of include/davidson_hip.h into every slot of A.lbound: min(LANCZOS_STEPS, n) steps, two fetched scalars each.  The three vectors
// rotate: u (then v), the product (then w, the next u), v_prev.  Products are timed and counted like any apply.
int lanczos_bound(E* e, OpDesc& A) {
  const int64_t ld = e->ldp;
  double* slots = e->lanczos_ws + 2 * ld;
  double* partial = slots + roundup(e->nranks, 2);
  double* buf[3] = {e->lanczos_ws, e->lanczos_ws + ld, e->cheb_ws + 2 * ws_block(e)};
  std::vector<double> host((size_t)e->nranks);
  hipStream_t st = e->stream;
  const int steps = (int)std::min<int64_t>(LANCZOS_STEPS, e->n);
  double nrm2 = 0.0;
  launch_lanczos_start(st, buf[0], e->row0, e->nloc, e->nloc_pad, partial, slots, e->rank, e->nranks);
  CHK(fetch_dot(e, slots, host, &nrm2));
  double nrm = std::sqrt(nrm2), beta = 0.0, amax = 0.0, bound = 0.0, beta_before = 0.0;
  int x = 0;                       // buf[x] = u, buf[(x + 1) % 3] takes the product, buf[(x + 2) % 3] = v_prev from the second step on
  for (int i = 0; i < steps; ++i) {
    double* u = buf[x];
    double* w = buf[(x + 1) % 3];
    const double* vprev = i > 0 ? buf[(x + 2) % 3] : nullptr;
    double alpha = 0.0, ww = 0.0;
    CHK(apply_ptr(e, DAV_OP_A, u, 1, w, true, false));
    launch_lanczos_first(st, u, w, vprev, nrm, beta, e->nloc, e->nloc_pad, partial, slots, e->rank, e->nranks);
    CHK(fetch_dot(e, slots, host, &alpha));
    launch_lanczos_second(st, w, u, alpha, e->nloc, e->nloc_pad, partial, slots, e->rank, e->nranks);
    CHK(fetch_dot(e, slots, host, &ww));
    beta_before = beta;
    beta = std::sqrt(ww);
    amax = nan_max(amax, std::fabs(alpha));
    const bool last = i + 1 == steps || beta <= 1e-12 * amax;
    // Gershgorin row i of the tridiagonal matrix (its last row has no beta_i), then the last beta on top of the maximum
    const double row = last ? alpha + beta_before : alpha + beta_before + beta;
    bound = i == 0 ? row : nan_max(bound, row);
    if (last) break;
    nrm = beta;
    x = (x + 1) % 3;
  }
  bound += beta;
  HIPCHK(hipGetLastError());
  std::fill(host.begin(), host.end(), bound);
  HIPCHK(hipMemcpyAsync(A.lbound, host.data(), sizeof(double) * (size_t)e->nranks, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));        // `host` goes out of scope
  return 0;
}

// the row-sum bound of the stored entries (CHEB) when it is stale - with several ranks one all-reduce
int row_sum_bound(E* e, OpDesc& A) {
  SparseStore& s = A.sp;
  if (s.rbound_valid) return 0;
  if (e->nranks > 1) CHK(need_comm(e));
  if (!s.rbound && pool_malloc(&s.rbound, sizeof(double) * (size_t)(e->nranks + CHEB_BOUND_PARTIALS)) != hipSuccess) {
    (void)hipGetLastError();
    s.rbound = nullptr;
    return refuse(DAV_METHOD_CHEB, "device memory for the spectral bound could not be allocated");
  }
  if (A.kind == DAV_KIND_DIA) launch_dia_row_bound(e->stream, s.dia_val, s.dia_ld, s.dia_nd, e->nloc, s.rbound + e->nranks, s.rbound, e->rank, e->nranks);
  else launch_cheb_row_bound(e->stream, s.b, s.rp, s.val, s.nrows, s.rbound + e->nranks, s.rbound, e->rank, e->nranks);
  HIPCHK(hipGetLastError());
  if (has_comm(e)) CHK(coll_allreduce(e, s.rbound, (size_t)e->nranks));     // a sum: every slot has one non-zero term
  s.rbound_valid = true;
  return 0;
}

// the Lanczos bound (LCHEB) when it is stale, behind its two vectors - every rank enters the collectives of the run
int lanczos_bound_ensure(E* e, OpDesc& A) {
  if (!e->lanczos_ws) {
    const size_t doubles = 2 * (size_t)e->ldp + (size_t)roundup(e->nranks, 2) + (size_t)lanczos_partials(e->nloc_pad);
    if (pool_malloc(&e->lanczos_ws, sizeof(double) * doubles) != hipSuccess) {
      (void)hipGetLastError();
      e->lanczos_ws = nullptr;
      return refuse(DAV_METHOD_LCHEB, "device memory for the two vectors of the Lanczos run could not be allocated");
    }
    HIPCHK(hipMemsetAsync(e->lanczos_ws, 0, sizeof(double) * doubles, e->stream));
  }
  if (!A.lbound && pool_malloc(&A.lbound, sizeof(double) * (size_t)e->nranks) != hipSuccess) {
    (void)hipGetLastError();
    A.lbound = nullptr;
    return refuse(DAV_METHOD_LCHEB, "device memory for the spectral bound could not be allocated");
  }
  if (!A.lbound_valid) {
    if (e->nranks > 1) CHK(need_comm(e));
    CHK(lanczos_bound(e, A));
    A.lbound_valid = true;
  }
  return 0;
}
}  // namespace

// What the method asks, decided from what this rank knows alone (every rank decides alike), in the order the refusals have always come:
// the problem, operator A, the degree; then the workspace and the bound of operator A when it is stale - every rank finds it stale at
// the same correction, so every rank enters the all-reduce (CHEB) or the collectives of the Lanczos run (LCHEB).  Called before the Ritz
// phase opens its event pair and before any panel is written: the products of the run are timed by their own pairs.
int cheb_prepare(E* e, const MethodSpec& method) {
  const int kind = method.kind, degree = method.degree;
  if (e->gev) return refuse(kind, "a generalized problem is not served (the filter would need the inverse of operator B)");
  OpDesc& A = e->op[DAV_OP_A];
  if (kind == DAV_METHOD_CHEB) {
    if (A.kind != DAV_KIND_CSR && A.kind != DAV_KIND_BSR && A.kind != DAV_KIND_DIA)
      return refuse(kind, std::string("operator A is ") + kind_words(A.kind) +
                          ": the spectral bound is taken from the stored entries of a CSR or BSR operator (dav_set_operator_csr / dav_set_operator_bsr)");
  } else {
    if (A.kind == DAV_KIND_NONE) return refuse(kind, "operator A is not set");
    if (A.kind == DAV_KIND_HOST)
      return refuse(kind, "operator A is a host callback: the engine cannot apply it on the device (dav_set_operator_device takes a device callback)");
  }
  if (degree < 1 || degree > CHEB_MAX_DEGREE) return refuse(kind, "degree " + std::to_string(degree) + " is outside 1.." + std::to_string(CHEB_MAX_DEGREE));
  CHK(ensure_workspace(e, kind));
  return kind == DAV_METHOD_CHEB ? row_sum_bound(e, A) : lanczos_bound_ensure(e, A);
}

// V[:, m:m+ncorr] = z_d from R[:, 0:ncorr] with the bound max(slots[0 .. nranks)) of the method - the row-sum bound of the stored operator
// or the Lanczos bound; cheb_prepare has passed - on the engine's stream behind the residual product that wrote R.  z_k alternate between workspace blocks; the last step writes into V.  Separate step: blocks 0 / 1 hold z, block 2 the product,
// the step overwrites z_{k-1} in place.  Fused (CSR, also stored by diagonals; DAV_CHEB_FUSE): the product's epilogue writes z_{k+1} into
// the third block, the three rotate.
int cheb_correct(E* e, const MethodSpec& method, int m, int ncorr, int lowest, const double* theta_dev) {
  if (ncorr > ws_cols(e)) return refuse(method.kind, "the correction block is wider than the workspace");
  const int degree = method.degree;
  const double* slots = method.kind == DAV_METHOD_CHEB ? e->op[DAV_OP_A].sp.rbound : e->op[DAV_OP_A].lbound;
  double* ws[3] = {e->cheb_ws, e->cheb_ws + ws_block(e), e->cheb_ws + 2 * ws_block(e)};
  double* coef = e->cheb_ws + 3 * ws_block(e);
  const int pstride = (int)roundup(ws_cols(e), 64);
  const double* R = panel_ptr(e, DAV_PANEL_R, 0);
  double* T = panel_ptr(e, DAV_PANEL_V, m);
  const int kind = e->op[DAV_OP_A].kind;
  const bool fuse = e->tune.cheb_fuse != 0 && (kind == DAV_KIND_CSR || kind == DAV_KIND_DIA);
  launch_cheb_coef(e->stream, theta_dev, ncorr, lowest, degree, slots, e->nranks, coef, pstride);
  launch_cheb_step(e->stream, 0, coef, pstride, nullptr, nullptr, R, nullptr, degree == 1 ? T : ws[0], e->ldp, ncorr, e->nloc, e->nloc_pad);
  int cur = 0, prev = -1;          // blocks of z_k and z_{k-1}
  for (int k = 1; k < degree; ++k) {
    const bool last = k + 1 == degree;
    const double* zprev = prev >= 0 ? ws[prev] : nullptr;
    if (fuse) {
      const int free_block = 3 - cur - (prev >= 0 ? prev : (cur == 0 ? 1 : 0));
      double* out = last ? T : ws[free_block];
      const ChebEpi epi{ws[cur], R, zprev, coef, coef + CHEB_AB + 2 * k, coef + CHEB_PI + (size_t)k * pstride, e->ldp};
      CHK(apply_csr_cheb(e, ws[cur], ncorr, out, epi));
      prev = cur; cur = free_block;
    } else {
      const int nxt = prev >= 0 ? prev : 1 - cur;        // z_{k+1} takes the place of z_{k-1}
      // (a sparse operator has no fp32 copy, so CHEB never saw the flag; LCHEB on dense tiles keeps fp64 whatever dav_set_inner_precision says)
      CHK(apply_ptr(e, DAV_OP_A, ws[cur], ncorr, ws[2], true, false));
      launch_cheb_step(e->stream, k, coef, pstride, ws[2], ws[cur], R, zprev, last ? T : ws[nxt], e->ldp, ncorr, e->nloc, e->nloc_pad);
      prev = cur; cur = nxt;
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}
