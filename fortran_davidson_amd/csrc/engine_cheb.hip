// Engine, the Chebyshev-filtered correction (DAV_METHOD_CHEB; include/davidson_hip.h states the recurrence and the interval): the contract
// of the method, the row-sum bound kept with a sparse operator, the workspace, and the step of the Ritz phase that turns the residues into
// the correction block by d - 1 block products (kernels in k_cheb.hip; the fused step of a CSR operator in k_spmm.hip).
#include "engine_internal.h"

namespace {
const char* kind_name(int kind) {
  switch (kind) {
    case DAV_KIND_NONE: return "not set";
    case DAV_KIND_DENSE: return "a dense matrix";
    case DAV_KIND_HOST: return "a host callback";
    case DAV_KIND_DEVICE: return "a device callback";
    case DAV_KIND_IDENTITY: return "the identity";
    default: return "a generated operator";
  }
}
int refuse(const std::string& why) { return fail("CHEB correction: " + why); }
int ws_cols(const E* e) { return e->cols_alloc / 2 + 8; }     // the width of a block of the GJD workspace
size_t ws_block(const E* e) { return (size_t)e->ldp * ws_cols(e); }
}  // namespace

// What the method asks, decided from what this rank knows alone (every rank decides alike); then the bound of operator A when it is stale -
// with several ranks one all-reduce, which every rank enters because every rank finds the bound stale at the same correction - and the
// workspace.  Nothing of the panels is written before this has passed.
int cheb_prepare(E* e, int degree) {
  if (e->gev) return refuse("a generalized problem is not served (the filter would need the inverse of operator B)");
  OpDesc& A = e->op[DAV_OP_A];
  if (A.kind != DAV_KIND_CSR && A.kind != DAV_KIND_BSR && A.kind != DAV_KIND_DIA)
    return refuse(std::string("operator A is ") + kind_name(A.kind) +
                  ": the spectral bound is taken from the stored entries of a CSR or BSR operator (dav_set_operator_csr / dav_set_operator_bsr)");
  if (degree < 1 || degree > CHEB_MAX_DEGREE) return refuse("degree " + std::to_string(degree) + " is outside 1.." + std::to_string(CHEB_MAX_DEGREE));
  if (!e->cheb_ws) {
    const size_t bytes = sizeof(double) * (3 * ws_block(e) + cheb_coef_doubles(ws_cols(e)));
    if (pool_malloc(&e->cheb_ws, bytes) != hipSuccess) {
      (void)hipGetLastError();
      e->cheb_ws = nullptr;
      return refuse("device memory for the workspace (" + std::to_string(bytes >> 20) + " MiB) could not be allocated");
    }
    HIPCHK(hipMemsetAsync(e->cheb_ws, 0, bytes, e->stream));
  }
  SparseStore& s = A.sp;
  if (!s.rbound_valid) {
    if (e->nranks > 1) CHK(need_comm(e));
    if (!s.rbound && pool_malloc(&s.rbound, sizeof(double) * (size_t)(e->nranks + CHEB_BOUND_PARTIALS)) != hipSuccess) {
      (void)hipGetLastError();
      s.rbound = nullptr;
      return refuse("device memory for the spectral bound could not be allocated");
    }
    if (A.kind == DAV_KIND_DIA) launch_dia_row_bound(e->stream, s.dia_val, s.dia_ld, s.dia_nd, e->nloc, s.rbound + e->nranks, s.rbound, e->rank, e->nranks);
    else launch_cheb_row_bound(e->stream, s.b, s.rp, s.val, s.nrows, s.rbound + e->nranks, s.rbound, e->rank, e->nranks);
    HIPCHK(hipGetLastError());
    if (has_comm(e)) CHK(coll_allreduce(e, s.rbound, (size_t)e->nranks));     // a sum: every slot has one non-zero term
    s.rbound_valid = true;
  }
  return 0;
}

// V[:, m:m+ncorr] = z_d from R[:, 0:ncorr] on the engine's stream, behind the residual product that wrote R (cheb_prepare has passed).
// z_k alternate between workspace blocks; the last step writes into V.  Separate step: blocks 0 / 1 hold z, block 2 the product, the step
// overwrites z_{k-1} in place.  Fused (CSR, also stored by diagonals; DAV_CHEB_FUSE): the product's epilogue writes z_{k+1} into the third block, the three rotate.
int cheb_correct(E* e, int m, int ncorr, int lowest, int degree, const double* theta_dev) {
  if (ncorr > ws_cols(e)) return refuse("the correction block is wider than the workspace");
  const SparseStore& s = e->op[DAV_OP_A].sp;
  double* ws[3] = {e->cheb_ws, e->cheb_ws + ws_block(e), e->cheb_ws + 2 * ws_block(e)};
  double* coef = e->cheb_ws + 3 * ws_block(e);
  const int pstride = (int)roundup(ws_cols(e), 64);
  const double* R = panel_ptr(e, DAV_PANEL_R, 0);
  double* T = panel_ptr(e, DAV_PANEL_V, m);
  const int kind = e->op[DAV_OP_A].kind;
  const bool fuse = e->tune.cheb_fuse != 0 && (kind == DAV_KIND_CSR || kind == DAV_KIND_DIA);
  launch_cheb_coef(e->stream, theta_dev, ncorr, lowest, degree, s.rbound, e->nranks, coef, pstride);
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
      CHK(apply_ptr(e, DAV_OP_A, ws[cur], ncorr, ws[2], true, true));
      launch_cheb_step(e->stream, k, coef, pstride, ws[2], ws[cur], R, zprev, last ? T : ws[nxt], e->ldp, ncorr, e->nloc, e->nloc_pad);
      prev = cur; cur = nxt;
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}
