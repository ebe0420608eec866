// Engine, the block-diagonal preconditioned correction (DAV_METHOD_BDPR): the contract of the method, the diagonal blocks kept with a BSR
// operator, and the step of the Ritz phase that turns the residues into the correction block (kernels in k_bdpr.hip).
#include "engine_internal.h"

namespace {
const char* slot_name(int which) { return which == DAV_OP_A ? "operator A" : "operator B"; }
int refuse(int which, const std::string& why) { return fail(std::string("BDPR correction: ") + slot_name(which) + " " + why); }
}  // namespace

// What the method asks of the operators, decided from what this rank knows alone (every rank decides alike, no collective), and the
// diagonal blocks of the operators that do not have theirs yet.  Nothing of the panels is written before this has passed.
int bdpr_prepare(E* e) {
  const OpDesc& A = e->op[DAV_OP_A];
  if (A.kind != DAV_KIND_BSR)
    return refuse(DAV_OP_A, std::string("is ") + kind_words(A.kind) + ": the block solves need the diagonal blocks of a BSR operator (dav_set_operator_bsr)");
  const int b = A.sp.b;
  if (e->gev) {
    const OpDesc& B = e->op[DAV_OP_B];
    if (B.kind != DAV_KIND_BSR)
      return refuse(DAV_OP_B, std::string("is ") + kind_words(B.kind) + ": a generalized problem needs a BSR operator B of the block size of A (" +
                                  std::to_string(b) + ")");
    if (B.sp.b != b)
      return refuse(DAV_OP_B, "has block size " + std::to_string(B.sp.b) + ", operator A has " + std::to_string(b) + ": the block sizes must be equal");
  }
  if (e->nranks > 1 && e->nslab % b != 0)
    return refuse(DAV_OP_A, "has block size " + std::to_string(b) + ", which does not divide the " + std::to_string(e->nslab) + " rows of a rank's slab (" +
                                std::to_string(e->nranks) + " ranks): a diagonal block would straddle two ranks");
  for (int w = 0; w < (e->gev ? 2 : 1); ++w) {
    SparseStore& s = e->op[w].sp;
    // (what the checks above imply: the local block rows are exactly this rank's rows)
    if (e->nloc > 0 && (s.grow0 != 0 || s.nrows * b != e->nloc)) return refuse(w, "keeps block rows that are not whole rows of this rank");
    if (s.bdiag_valid || e->nloc == 0) continue;
    const size_t count = (size_t)s.nrows * b * b;
    if (!s.bdiag && pool_malloc(&s.bdiag, sizeof(double) * std::max<size_t>(count, 1)) != hipSuccess) {
      (void)hipGetLastError();
      s.bdiag = nullptr;
      return refuse(w, "device memory for the diagonal blocks (" + std::to_string((sizeof(double) * count) >> 20) + " MiB) could not be allocated");
    }
    launch_bdpr_diag_blocks(e->stream, b, s.rp, s.col, s.val, s.nrows, e->row0 / b, s.bdiag);
    HIPCHK(hipGetLastError());
    s.bdiag_valid = true;
  }
  return 0;
}

// V[:, m:m+ncorr] = blocksolve(R[:, 0:ncorr]) on the engine's stream, behind the residual product that wrote R (bdpr_prepare has passed)
void bdpr_correct(E* e, int m, int ncorr, const double* theta_dev) {
  const SparseStore& a = e->op[DAV_OP_A].sp;
  launch_bdpr_solve(e->stream, a.b, a.bdiag, e->gev ? e->op[DAV_OP_B].sp.bdiag : nullptr, theta_dev, panel_ptr(e, DAV_PANEL_R, 0), e->ldp,
                    panel_ptr(e, DAV_PANEL_V, m), e->ldp, ncorr, a.nrows, e->nloc, e->nloc_pad);
}
