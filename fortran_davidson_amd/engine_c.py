"""Thin ctypes view of the C ABI (include/davidson_hip.h) - used by the kernel-level parity tests
and by bench.py for the roofline measurement.  One method per C entry point, numpy in/out."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import hip_lib

OP_A, OP_B = 0, 1
# DAV_OP_M: the caller's preconditioner, an approximation of (A - sigma B)^-1 that DPR and GJD apply (include/davidson_hip.h).  The sparse,
# device-callback and identity entries, keep_value_map / update_operator_values / get_diagonal and apply(_inner) take it; the dense, hashed,
# harness and host entries refuse it (DavidsonHipError naming DAV_OP_M).  BDPR, CHEB and LCHEB do not read it; there is no unset.
OP_M = 2
PANEL_V, PANEL_W, PANEL_BV, PANEL_X, PANEL_R, PANEL_S = range(6)
# the method codes (the header's DAV_METHOD_*); a new method is one row here
METHOD_DPR, METHOD_GJD, METHOD_NONE = 0, 1, 2
METHOD_BDPR = 3          # block-diagonal DPR of a BSR operator
METHOD_CHEB = 4          # Chebyshev-filtered correction of a CSR / BSR operator, default degree
METHOD_LCHEB = 5         # the same correction with a Lanczos bound, for any operator applied on the device


def method_code(kind, degree=0):
    """the method code of `kind` with the degree of the Chebyshev corrections in bits 8..15 (the header's DAV_METHOD_CHEB_DEGREE /
    DAV_METHOD_LCHEB_DEGREE), 0 = the engine's default of 10.  The engine itself refuses a degree outside 1..64."""
    return kind | (int(degree) << 8)


def method_cheb(degree=0):
    return method_code(METHOD_CHEB, degree)


def method_lcheb(degree=0):
    return method_code(METHOD_LCHEB, degree)


# int fn(ctx, hip_stream, n, row0, nloc, k, x_dev, ldx, y_dev, ldy) - include/davidson_hip.h: dav_device_apply_fn
DEVICE_APPLY_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64)


class DavidsonHipError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [("n", C.c_int64), ("nloc", C.c_int64), ("nranks", C.c_int32), ("rank", C.c_int32),
                ("m", C.c_int32), ("applies", C.c_int32), ("apply_cols", C.c_int64),
                ("apply_ms", C.c_double), ("apply_bytes", C.c_double), ("last_apply_ms", C.c_double),
                ("last_apply_bytes", C.c_double), ("gram_ms", C.c_double), ("panel_ms", C.c_double),
                ("comm_ms", C.c_double), ("apply_kernel_ms", C.c_double), ("apply_flops", C.c_double),
                ("apply_launches", C.c_int64), ("restarts", C.c_int64),
                ("allgather_ms", C.c_double), ("reduce_scatter_ms", C.c_double), ("allreduce_ms", C.c_double),
                ("allgather_bytes", C.c_double), ("reduce_scatter_bytes", C.c_double), ("allreduce_bytes", C.c_double),
                ("collectives", C.c_int64), ("comm_ranks", C.c_int32), ("comm_overlap", C.c_int32), ("apply_comm_ms", C.c_double),
                ("b_stored_kernel_ms", C.c_double), ("b_stored_bytes", C.c_double), ("b_stored_flops", C.c_double),
                ("b_generated_kernel_ms", C.c_double), ("b_generated_entries", C.c_double), ("b_generated_flops", C.c_double),
                ("b_stored_launches", C.c_int64), ("b_generated_launches", C.c_int64)]


ABI_VERSION = 109      # DAV_HIP_ABI_VERSION of include/davidson_hip.h this module mirrors


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


CSR_FULL, CSR_LOWER = 0, 1
CSR_DIAGONALS = 2          # or-ed to either: the matrix is stored by diagonals (DAV_CSR_DIAGONALS)


def csr_flag_word(lower=False, diagonals=False):
    """the `triangle` argument of the CSR set entries (and the `lower` integer of the Fortran doors): bit 0 lower, bit 1 diagonals"""
    return (CSR_LOWER if lower else CSR_FULL) | (CSR_DIAGONALS if diagonals else 0)


def csr_arrays(indptr, indices=None, data=None, n=None):
    """(indptr int64, indices int32, data float64) of a CSR matrix given as three arrays or as one object with .tocsr() (a scipy
    sparse matrix; scipy itself is never imported here).  Checks only what keeps the C call inside the arrays: n + 1 offsets, at least
    indptr[-1] - indptr[0] entries."""
    if hasattr(indptr, "tocsr"):
        m = indptr.tocsr()
        indptr, indices, data = m.indptr, m.indices, m.data
    if indices is None or data is None:
        raise DavidsonHipError("CSR input: indptr, indices and data are all needed (or one object with .tocsr())")
    rp = np.ascontiguousarray(indptr, dtype=np.int64)
    ci = np.ascontiguousarray(indices)
    if ci.size and (ci.min() < -2**31 or ci.max() >= 2**31):
        raise DavidsonHipError("CSR input: column indices do not fit int32")
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    vv = np.ascontiguousarray(data, dtype=np.float64)
    if rp.ndim != 1 or (n is not None and rp.size != n + 1) or rp.size < 2:
        raise DavidsonHipError(f"CSR input: indptr must hold n + 1 = {'?' if n is None else n + 1} offsets, it holds {rp.size}")
    nnz = int(rp[-1] - rp[0])
    if nnz < 0 or ci.size < nnz or vv.size < nnz:
        raise DavidsonHipError(f"CSR input: indptr says {nnz} entries, indices / data hold {ci.size} / {vv.size}")
    return rp, ci, vv


def is_torch_csr(t):
    """True for a torch tensor in the sparse CSR layout (torch itself is imported only when the object comes from it)"""
    if not type(t).__module__.startswith("torch"):
        return False
    import torch
    return isinstance(t, torch.Tensor) and t.layout == torch.sparse_csr


def device_csr_tensors(row_ptr, col_idx, vals, n, device):
    """The checks of a CSR matrix in device tensors before any library call: int32 / int64 indices and float64 values (TypeError, never
    converted), contiguous tensors on cuda:`device` and n + 1 offsets (ValueError).  Returns (row_ptr_bits, col_bits)."""
    return _device_csr_tensors(row_ptr, col_idx, vals, n, device)[:2]


def _device_csr_tensors(row_ptr, col_idx, vals, n, device):
    """device_csr_tensors, with the number of entries row_ptr gives as a third result"""
    import torch
    args = (("row_ptr", row_ptr, (torch.int32, torch.int64)), ("col_idx", col_idx, (torch.int32, torch.int64)),
            ("vals", vals, (torch.float64,)))
    for name, t, kinds in args:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"device CSR input: {name} must be a torch tensor, not {type(t).__name__}")
        if t.dtype not in kinds:
            raise TypeError(f"device CSR input: {name} has dtype {t.dtype}, expected " + " or ".join(str(k) for k in kinds))
    for name, t, _ in args:
        if t.layout != torch.strided or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"device CSR input: {name} must be a contiguous one-dimensional tensor")
    for name, t, _ in args:
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError(f"device CSR input: {name} lies on {t.device}, the engine on cuda:{device}")
    if row_ptr.numel() != n + 1:
        raise ValueError(f"device CSR input: row_ptr must hold n + 1 = {n + 1} offsets, it holds {row_ptr.numel()}")
    nnz = int(row_ptr[-1]) - int(row_ptr[0])          # two values read back: the kernels must not read past the tensors
    if col_idx.numel() < nnz or vals.numel() < nnz:
        raise ValueError(f"device CSR input: row_ptr says {nnz} entries, col_idx / vals hold {col_idx.numel()} / {vals.numel()}")
    return (64 if row_ptr.dtype == torch.int64 else 32), (64 if col_idx.dtype == torch.int64 else 32), nnz


def torch_csr_parts(t):
    """(crow_indices, col_indices, values) of a torch sparse CSR tensor; on the CPU as numpy arrays"""
    if t.dim() != 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f"CSR input: a square matrix is needed, the tensor has shape {tuple(t.shape)}")
    parts = (t.crow_indices(), t.col_indices(), t.values())
    if t.device.type == "cpu":
        return tuple(x.numpy() for x in parts)
    return parts


def check_csr(indptr, indices, data, n, base=0, lower=False):
    """Everything dav_set_operator_csr validates, checked in Python (ValueError) - for the Fortran doors, which stop the process on an
    engine error.  Returns the arrays as csr_arrays does."""
    try:
        rp, ci, vv = csr_arrays(indptr, indices, data, n)
    except DavidsonHipError as exc:
        raise ValueError(str(exc)) from None
    if base not in (0, 1):
        raise ValueError("CSR input: index base must be 0 or 1")
    if rp[0] != base:
        raise ValueError(f"CSR input: indptr[0] = {rp[0]} must equal the index base {base}")
    if np.any(np.diff(rp) < 0):
        raise ValueError(f"CSR input: indptr decreases at row {int(np.argmax(np.diff(rp) < 0)) + base}")
    nnz = int(rp[-1] - base)
    cols = ci[:nnz].astype(np.int64) - base
    if nnz and (cols.min() < 0 or cols.max() >= n):
        raise ValueError(f"CSR input: column index out of range [{base}, {n + base})")
    if lower and nnz:
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        if np.any(cols > rows):
            p = int(np.argmax(cols > rows))
            raise ValueError(f"CSR input: entry ({rows[p] + base}, {cols[p] + base}) lies above the diagonal with lower=True")
    return rp, ci, vv


def hermitian_arrays(indptr, indices=None, data=None, n=None):
    """(indptr int64, indices int32, data complex128) of a complex Hermitian CSR matrix of order n given as three arrays, as one object
    with .indptr, .indices and .data (a scipy csr_matrix of complex dtype, read as it stands; scipy itself is never imported here) or
    as a complex torch.sparse_csr_tensor on the CPU.  complex128 values are handed over as they lie - no copy, no expansion into real
    blocks: the engine reads the (re, im) pairs of the array itself.  Other dtypes are a TypeError (never converted).  Checks only
    what keeps the C call inside the arrays."""
    if is_torch_csr(indptr):
        indptr, indices, data = torch_csr_parts(indptr)
    elif indices is None and data is None and all(hasattr(indptr, name) for name in ("indptr", "indices", "data")):
        indptr, indices, data = indptr.indptr, indptr.indices, indptr.data
    if indices is None or data is None:
        raise DavidsonHipError("Hermitian CSR input: indptr, indices and data are all needed (or one object with .indptr, .indices and .data)")
    vv = np.asarray(data)
    if vv.dtype != np.complex128:
        raise TypeError(f"Hermitian CSR input: data has dtype {vv.dtype}, expected complex128")
    vv = np.ascontiguousarray(vv)
    rp = np.ascontiguousarray(indptr, dtype=np.int64)
    ci = np.ascontiguousarray(indices)
    if ci.size and (ci.min() < -2**31 or ci.max() >= 2**31):
        raise DavidsonHipError("Hermitian CSR input: column indices do not fit int32")
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    if rp.ndim != 1 or (n is not None and rp.size != n + 1) or rp.size < 2:
        raise DavidsonHipError(f"Hermitian CSR input: indptr must hold n + 1 = {'?' if n is None else n + 1} offsets, it holds {rp.size}")
    nnz = int(rp[-1] - rp[0])
    if nnz < 0 or ci.size < nnz or vv.size < nnz or vv.ndim != 1:
        raise DavidsonHipError(f"Hermitian CSR input: indptr says {nnz} entries, indices / data hold {ci.size} / {vv.size}")
    return rp, ci, vv


def check_hermitian(indptr, indices, data, n, base=0, lower=False):
    """Everything davh_set_operator_csr validates, checked in Python (ValueError) - for the Fortran doors, which stop the process on an
    engine error.  Returns the arrays as hermitian_arrays does."""
    try:
        rp, ci, vv = hermitian_arrays(indptr, indices, data, n)
    except DavidsonHipError as exc:
        raise ValueError(str(exc)) from None
    if base not in (0, 1):
        raise ValueError("Hermitian CSR input: index base must be 0 or 1")
    if rp[0] != base:
        raise ValueError(f"Hermitian CSR input: indptr[0] = {rp[0]} must equal the index base {base}")
    if np.any(np.diff(rp) < 0):
        raise ValueError(f"Hermitian CSR input: indptr decreases at row {int(np.argmax(np.diff(rp) < 0)) + base}")
    nnz = int(rp[-1] - base)
    cols = ci[:nnz].astype(np.int64) - base
    if nnz and (cols.min() < 0 or cols.max() >= n):
        raise ValueError(f"Hermitian CSR input: column index out of range [{base}, {n + base})")
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    if lower and np.any(cols > rows):
        p = int(np.argmax(cols > rows))
        raise ValueError(f"Hermitian CSR input: entry ({rows[p] + base}, {cols[p] + base}) lies above the diagonal with lower=True")
    bad = (cols == rows) & ~(vv[:nnz].imag == 0.0)
    if bad.any():
        p = int(np.argmax(bad))
        raise ValueError(f"Hermitian CSR input: diagonal entry {p + base} (row {rows[p] + base}) has the imaginary part "
                         f"{float(vv[p].imag)!r}: the diagonal of a Hermitian matrix is real")
    return rp, ci, vv


def _device_hermitian_tensors(row_ptr, col_idx, vals, n, device):
    """The checks of a complex CSR matrix of order n in device tensors before any library call: int32 / int64 indices and complex128
    values (TypeError, never converted), contiguous tensors on cuda:`device`, n + 1 offsets (ValueError).  Returns (row_ptr_bits,
    col_bits, nnz)."""
    import torch
    args = (("row_ptr", row_ptr, (torch.int32, torch.int64)), ("col_idx", col_idx, (torch.int32, torch.int64)),
            ("vals", vals, (torch.complex128,)))
    for name, t, kinds in args:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"device Hermitian CSR input: {name} must be a torch tensor, not {type(t).__name__}")
        if t.dtype not in kinds:
            raise TypeError(f"device Hermitian CSR input: {name} has dtype {t.dtype}, expected " + " or ".join(str(k) for k in kinds))
    for name, t, _ in args:
        if t.layout != torch.strided or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"device Hermitian CSR input: {name} must be a contiguous one-dimensional tensor")
    for name, t, _ in args:
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError(f"device Hermitian CSR input: {name} lies on {t.device}, the engine on cuda:{device}")
    if row_ptr.numel() != n + 1:
        raise ValueError(f"device Hermitian CSR input: row_ptr must hold n + 1 = {n + 1} offsets, it holds {row_ptr.numel()}")
    nnz = int(row_ptr[-1]) - int(row_ptr[0])          # two values read back: the kernels must not read past the tensors
    if col_idx.numel() < nnz or vals.numel() < nnz:
        raise ValueError(f"device Hermitian CSR input: row_ptr says {nnz} entries, col_idx / vals hold {col_idx.numel()} / {vals.numel()}")
    return (64 if row_ptr.dtype == torch.int64 else 32), (64 if col_idx.dtype == torch.int64 else 32), nnz


def is_torch_coo(t):
    """True for a torch tensor in the sparse COO layout (torch itself is imported only when the object comes from it)"""
    if not type(t).__module__.startswith("torch"):
        return False
    import torch
    return isinstance(t, torch.Tensor) and t.layout == torch.sparse_coo


def torch_coo_parts(t):
    """(rows, cols, values) of a torch sparse COO tensor AS THEY STAND - _indices() and _values(), coalesced or not, duplicates
    included; on the CPU as numpy arrays"""
    if t.dim() != 2 or t.shape[0] != t.shape[1] or t.dense_dim() != 0:
        raise ValueError(f"COO input: a square matrix of scalars is needed, the tensor has shape {tuple(t.shape)}")
    idx, vals = t._indices(), t._values()
    parts = (idx[0].contiguous(), idx[1].contiguous(), vals.contiguous())
    if t.device.type == "cpu":
        return tuple(x.numpy() for x in parts)
    return parts


def coo_triples(rows, cols=None, vals=None):
    """(rows, cols, vals) of COO input as it stands: three arrays, or one object with .row, .col and .data (a scipy coo_matrix - read
    without sum_duplicates() and without tocsr(); scipy itself is never imported here), or a torch.sparse_coo_tensor.  Torch tensors
    on the CPU - the parts of a COO tensor, or three tensors given one by one - come back as numpy arrays (the host path); tensors on a
    GPU stay tensors (the device path)."""
    def host(a):
        if type(a).__module__.startswith("torch") and hasattr(a, "device") and a.device.type == "cpu":
            return a.detach().contiguous().numpy()
        return a
    if cols is None and vals is None:
        if is_torch_coo(rows):
            return torch_coo_parts(rows)
        if all(hasattr(rows, name) for name in ("row", "col", "data")):
            return rows.row, rows.col, rows.data
    if cols is None or vals is None:
        raise DavidsonHipError("COO input: rows, cols and vals are all needed (or one object with .row, .col and .data, or a "
                               "torch.sparse_coo_tensor)")
    return host(rows), host(cols), host(vals)


def coo_arrays(rows, cols=None, vals=None):
    """(rows int32, cols int32, vals float64) of COO input in host memory (coo_triples says what is accepted), the triples in their
    order.  Checks only what keeps the C call inside the arrays: three one-dimensional arrays of one length.  An index that does not
    fit int32 becomes -2^31 or 2^31 - 1, which the engine refuses as out of range at that triple."""
    rows, cols, vals = coo_triples(rows, cols, vals)
    out = []
    for a in (rows, cols):
        a = np.ascontiguousarray(a)
        if a.dtype.kind not in "iu":
            raise DavidsonHipError(f"COO input: indices must be integers, not {a.dtype}")
        if a.dtype != np.int32:
            a = np.clip(a, -2**31 if a.dtype.kind == "i" else 0, 2**31 - 1).astype(np.int32)
        out.append(a)
    vv = np.ascontiguousarray(vals, dtype=np.float64)
    if any(a.ndim != 1 for a in (*out, vv)) or not out[0].size == out[1].size == vv.size:
        raise DavidsonHipError(f"COO input: rows / cols / vals hold {out[0].size} / {out[1].size} / {vv.size} values: three "
                               "one-dimensional arrays of one length are needed")
    return out[0], out[1], vv


def check_coo(rows, cols, vals, n, base=0, lower=False):
    """Everything davx_set_operator_coo validates, checked in Python (ValueError) - for the Fortran doors, which stop the process on an
    engine error.  Returns the arrays as coo_arrays does."""
    try:
        ri, ci, vv = coo_arrays(rows, cols, vals)
    except DavidsonHipError as exc:
        raise ValueError(str(exc)) from None
    if base not in (0, 1):
        raise ValueError("COO input: index base must be 0 or 1")
    if vv.size >= 2**32:
        raise ValueError("COO input: fewer than 2^32 triples are needed")
    i, j = ri.astype(np.int64) - base, ci.astype(np.int64) - base
    bad = (i < 0) | (i >= n) | (j < 0) | (j >= n) | ((j > i) if lower else False)
    if bad.any():
        p = int(np.argmax(bad))
        what = "lies above the diagonal with lower=True" if 0 <= i[p] < n and 0 <= j[p] < n else f"is out of range [{base}, {n + base})"
        raise ValueError(f"COO input: triple {p + base} at ({ri[p]}, {ci[p]}) {what}")
    return ri, ci, vv


def _device_coo_tensors(rows, cols, vals, device):
    """The checks of COO triples in device tensors before any library call: int32 / int64 indices and float64 values (TypeError, never
    converted), contiguous one-dimensional tensors of one length on cuda:`device` (ValueError).  Returns (row_bits, col_bits, nnz)."""
    import torch
    args = (("rows", rows, (torch.int32, torch.int64)), ("cols", cols, (torch.int32, torch.int64)), ("vals", vals, (torch.float64,)))
    for name, t, kinds in args:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"device COO input: {name} must be a torch tensor, not {type(t).__name__}")
        if t.dtype not in kinds:
            raise TypeError(f"device COO input: {name} has dtype {t.dtype}, expected " + " or ".join(str(k) for k in kinds))
    for name, t, _ in args:
        if t.layout != torch.strided or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"device COO input: {name} must be a contiguous one-dimensional tensor")
    for name, t, _ in args:
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError(f"device COO input: {name} lies on {t.device}, the engine on cuda:{device}")
    if not rows.numel() == cols.numel() == vals.numel():
        raise ValueError(f"device COO input: rows / cols / vals hold {rows.numel()} / {cols.numel()} / {vals.numel()} values")
    return (64 if rows.dtype == torch.int64 else 32), (64 if cols.dtype == torch.int64 else 32), vals.numel()


BSR_ROW_MAJOR, BSR_COL_MAJOR = 0, 1


def bsr_arrays(indptr, indices=None, data=None, n=None, layout=BSR_ROW_MAJOR):
    """(b, indptr int64, indices int32, data float64 of shape (nnzb, b, b)) of a BSR matrix given as three arrays - data (nnzb, b, b),
    each block in `layout` order (row-major: data[p, m, k] = A_p[m, k]) - or as one object with .indptr, .indices, .data and .blocksize
    (a scipy bsr_matrix, duck-typed; scipy is never imported here).  Checks only what keeps the C call inside the arrays."""
    if hasattr(indptr, "blocksize"):
        m = indptr
        indptr, indices, data = m.indptr, m.indices, m.data
        if tuple(m.blocksize)[0] != tuple(m.blocksize)[-1]:
            raise DavidsonHipError(f"BSR input: blocks must be square, blocksize = {tuple(m.blocksize)}")
    if indices is None or data is None:
        raise DavidsonHipError("BSR input: indptr, indices and data are all needed (or one object with .blocksize)")
    vv = np.ascontiguousarray(data, dtype=np.float64)
    if vv.ndim != 3 or vv.shape[1] != vv.shape[2]:
        raise DavidsonHipError(f"BSR input: data must have shape (nnzb, b, b), it has {vv.shape}")
    b = int(vv.shape[1])
    rp = np.ascontiguousarray(indptr, dtype=np.int64)
    ci = np.ascontiguousarray(indices)
    if ci.size and (ci.min() < -2**31 or ci.max() >= 2**31):
        raise DavidsonHipError("BSR input: block column indices do not fit int32")
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    if b < 1 or b > 16:
        raise DavidsonHipError(f"BSR input: block size {b} must lie in 1..16")
    if n is not None and n % b:
        raise DavidsonHipError(f"BSR input: n = {n} is not a multiple of the block size {b}")
    if rp.ndim != 1 or (n is not None and rp.size != n // b + 1) or rp.size < 2:
        raise DavidsonHipError(f"BSR input: indptr must hold n / b + 1 = {'?' if n is None else n // b + 1} offsets, it holds {rp.size}")
    nnzb = int(rp[-1] - rp[0])
    if nnzb < 0 or ci.size < nnzb or vv.shape[0] < nnzb:
        raise DavidsonHipError(f"BSR input: indptr says {nnzb} blocks, indices / data hold {ci.size} / {vv.shape[0]}")
    if layout not in (BSR_ROW_MAJOR, BSR_COL_MAJOR):
        raise DavidsonHipError("BSR input: layout must be BSR_ROW_MAJOR (0) or BSR_COL_MAJOR (1)")
    return b, rp, ci, vv


def check_bsr(indptr, indices, data, n, base=0, lower=False, layout=BSR_ROW_MAJOR):
    """Everything dav_set_operator_bsr validates, checked in Python (ValueError) - for the Fortran doors, which stop the process on an
    engine error.  Returns (b, indptr, indices, data) as bsr_arrays does."""
    try:
        b, rp, ci, vv = bsr_arrays(indptr, indices, data, n, layout)
    except DavidsonHipError as exc:
        raise ValueError(str(exc)) from None
    nb = n // b
    if base not in (0, 1):
        raise ValueError("BSR input: index base must be 0 or 1")
    if rp[0] != base:
        raise ValueError(f"BSR input: indptr[0] = {rp[0]} must equal the index base {base}")
    if np.any(np.diff(rp) < 0):
        raise ValueError(f"BSR input: indptr decreases at block row {int(np.argmax(np.diff(rp) < 0)) + base}")
    nnzb = int(rp[-1] - base)
    cols = ci[:nnzb].astype(np.int64) - base
    if nnzb and (cols.min() < 0 or cols.max() >= nb):
        raise ValueError(f"BSR input: block column index out of range [{base}, {nb + base})")
    if lower and nnzb:
        rows = np.repeat(np.arange(nb, dtype=np.int64), np.diff(rp))
        if np.any(cols > rows):
            p = int(np.argmax(cols > rows))
            raise ValueError(f"BSR input: block ({rows[p] + base}, {cols[p] + base}) lies above the diagonal with lower=True")
    return b, rp, ci, vv


def is_torch_bsr(t):
    """True for a torch tensor in the sparse BSR layout (torch itself is imported only when the object comes from it)"""
    if not type(t).__module__.startswith("torch"):
        return False
    import torch
    return isinstance(t, torch.Tensor) and t.layout == torch.sparse_bsr


def torch_bsr_parts(t):
    """(crow_indices, col_indices, values (nnzb, b, b), row-major blocks) of a torch sparse BSR tensor; on the CPU as numpy arrays"""
    if t.dim() != 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f"BSR input: a square matrix is needed, the tensor has shape {tuple(t.shape)}")
    parts = (t.crow_indices(), t.col_indices(), t.values())
    if t.device.type == "cpu":
        return tuple(x.numpy() for x in parts)
    return parts


def device_bsr_tensors(row_ptr, col_idx, vals, n, device):
    """The checks of a BSR matrix in device tensors before any library call: int32 / int64 indices and float64 values (TypeError, never
    converted); contiguous tensors on cuda:`device`, vals of shape (nnzb, b, b) with 1 <= b <= 16 dividing n, n / b + 1 offsets and
    enough block columns and blocks (ValueError).  Returns (b, row_ptr_bits, col_bits)."""
    return _device_bsr_tensors(row_ptr, col_idx, vals, n, device)[:3]


def _device_bsr_tensors(row_ptr, col_idx, vals, n, device):
    """device_bsr_tensors, with the number of blocks row_ptr gives as a fourth result"""
    import torch
    args = (("row_ptr", row_ptr, (torch.int32, torch.int64), 1), ("col_idx", col_idx, (torch.int32, torch.int64), 1),
            ("vals", vals, (torch.float64,), 3))
    for name, t, kinds, _ in args:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"device BSR input: {name} must be a torch tensor, not {type(t).__name__}")
        if t.dtype not in kinds:
            raise TypeError(f"device BSR input: {name} has dtype {t.dtype}, expected " + " or ".join(str(k) for k in kinds))
    for name, t, _, dims in args:
        if t.layout != torch.strided or not t.is_contiguous() or t.dim() != dims:
            raise ValueError(f"device BSR input: {name} must be a contiguous tensor of {dims} dimension{'s' if dims > 1 else ''}")
    for name, t, _, _ in args:
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError(f"device BSR input: {name} lies on {t.device}, the engine on cuda:{device}")
    if vals.shape[1] != vals.shape[2]:
        raise ValueError(f"device BSR input: vals must have shape (nnzb, b, b), it has {tuple(vals.shape)}")
    b = int(vals.shape[1])
    if b < 1 or b > 16:
        raise ValueError(f"device BSR input: block size {b} must lie in 1..16")
    if n % b:
        raise ValueError(f"device BSR input: n = {n} is not a multiple of the block size {b}")
    if row_ptr.numel() != n // b + 1:
        raise ValueError(f"device BSR input: row_ptr must hold n / b + 1 = {n // b + 1} offsets, it holds {row_ptr.numel()}")
    nnzb = int(row_ptr[-1]) - int(row_ptr[0])         # two values read back: the kernels must not read past the tensors
    if col_idx.numel() < nnzb or vals.shape[0] < nnzb:
        raise ValueError(f"device BSR input: row_ptr says {nnzb} blocks, col_idx / vals hold {col_idx.numel()} / {vals.shape[0]}")
    return b, (64 if row_ptr.dtype == torch.int64 else 32), (64 if col_idx.dtype == torch.int64 else 32), nnzb


def update_values_array(vals, count, device=None, what="update_operator_values", pairs=False):
    """The checks of new values for a kept pattern before any library call: float64 (TypeError, never converted), contiguous, and - where
    `count` (the values the set call saw) is known - exactly that many (ValueError); BSR blocks as (nnzb, b, b) or flat.  pairs: the
    operator is a Hermitian one (set_operator_csr_hermitian): complex128 instead, one value per entry; a real operator takes no
    complex values and a Hermitian one no real ones (TypeError).  Returns (flat numpy array, None) for host data (numpy, or a torch
    tensor on the CPU) or (None, torch tensor) for a tensor on cuda:`device`."""
    if type(vals).__module__.startswith("torch"):
        import torch
        if vals.dtype != (torch.complex128 if pairs else torch.float64):
            raise TypeError(f"{what}: vals has dtype {vals.dtype}, expected " + ("torch.complex128" if pairs else "torch.float64"))
        if vals.layout != torch.strided or not vals.is_contiguous():
            raise ValueError(f"{what}: vals must be a contiguous tensor")
        if count is not None and vals.numel() != count:
            raise ValueError(f"{what}: the set call saw {count} values, vals holds {vals.numel()}")
        if vals.device.type == "cpu":
            return vals.numpy().reshape(-1), None
        if vals.device.type != "cuda" or (device is not None and vals.device.index != device):
            raise ValueError(f"{what}: vals lies on {vals.device}, the engine on cuda:{device}")
        return None, vals
    a = np.asarray(vals)
    if a.dtype != (np.complex128 if pairs else np.float64):
        raise TypeError(f"{what}: vals has dtype {a.dtype}, expected " + ("complex128" if pairs else "float64"))
    if count is not None and a.size != count:
        raise ValueError(f"{what}: the set call saw {count} values, vals holds {a.size}")
    return np.ascontiguousarray(a).reshape(-1), None


def guess_array(x, n, device=None, what="set_guess"):
    """The checks of an initial guess before any library call: float64 (TypeError, never converted), two-dimensional - one column per
    vector; a one-dimensional array is one column - with n rows (ValueError).  Returns (Fortran-ordered numpy array, None) for host data
    (numpy, or a torch tensor on the CPU) or (None, (tensor, ldx, ncols)) for a torch tensor on cuda:`device`: a column-major view or
    copy whose columns lie ldx doubles apart."""
    if type(x).__module__.startswith("torch"):
        import torch
        if x.dtype != torch.float64:
            raise TypeError(f"{what}: x has dtype {x.dtype}, expected torch.float64")
        if x.dim() == 1:
            x = x.reshape(-1, 1)
        if x.dim() != 2 or x.shape[0] != n or x.shape[1] < 1:
            raise ValueError(f"{what}: x must have shape ({n}, ncols), it has {tuple(x.shape)}")
        if x.device.type == "cpu":
            return np.asfortranarray(x.numpy()), None
        if x.device.type != "cuda" or (device is not None and x.device.index != device):
            raise ValueError(f"{what}: x lies on {x.device}, the engine on cuda:{device}")
        ncols = x.shape[1]
        if not (x.stride(0) == 1 and (ncols == 1 or x.stride(1) >= n)):
            x = x.t().contiguous().t()                 # column-major copy
        return None, (x, n if ncols == 1 else x.stride(1), ncols)
    a = np.asarray(x)
    if a.dtype != np.float64:
        raise TypeError(f"{what}: x has dtype {a.dtype}, expected float64")
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2 or a.shape[0] != n or a.shape[1] < 1:
        raise ValueError(f"{what}: x must have shape ({n}, ncols), it has {a.shape}")
    return np.asfortranarray(a), None


def _f(a):
    return np.asfortranarray(a, dtype=np.float64)


def _optional(x):
    """(use_x, x) as the C side takes an optional double: `int use_x, double x`"""
    return (0, 0.0) if x is None else (1, x)


class CEngine:
    """RAII wrapper over dav_create/dav_destroy.  `handle` may be borrowed from the Fortran side."""

    def __init__(self, n=None, max_cols=None, gev=False, device=0, rank=0, nranks=1, handle=None):
        self.lib = hip_lib()
        if self.lib.dav_version() != ABI_VERSION:
            raise DavidsonHipError(f"libdavidson_hip.so reports ABI version {self.lib.dav_version()}, engine_c.py mirrors {ABI_VERSION}")
        self.owned = handle is None
        if handle is None:
            h = C.c_void_p()
            self._chk(self.lib.dav_create(C.byref(h), device, n, max_cols, int(gev), rank, nranks))
            self.h = h
        else:
            self.h = C.c_void_p(handle)
        self.device = device
        st = self.stats()
        self.n = st.n

    def _chk(self, rc):
        if rc != 0:
            raise DavidsonHipError(self.lib.dav_last_error().decode())

    def close(self):
        if self.owned and self.h:
            self.lib.dav_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- bookkeeping
    def stats(self) -> Stats:
        st = Stats()
        self._chk(self.lib.dav_get_stats_n(self.h, C.byref(st), C.sizeof(st)))
        return st

    def reset_stats(self):
        self._chk(self.lib.dav_reset_stats(self.h))

    def set_timing(self, level):
        """0 = no events, 1 = block matvec only (default), 2 = every phase (gram_ms, panel_ms, comm_ms)."""
        self._chk(self.lib.dav_set_timing(self.h, level))

    def synchronize(self):
        self._chk(self.lib.dav_synchronize(self.h))

    def local_rows(self):
        r0, nl = C.c_int64(), C.c_int64()
        self._chk(self.lib.dav_local_rows(self.h, C.byref(r0), C.byref(nl)))
        return r0.value, nl.value

    def comm_init(self, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, 128)
        self._chk(self.lib.dav_comm_init(self.h, buf))

    def comm_path(self):
        """What the trial of the collective paths decided (dav_comm_path): dict(selected, trial_ran, columns, ms, valid)"""
        sel, ran, cols = C.c_int(), C.c_int(), C.c_int()
        ms = (C.c_double * 3)()
        valid = (C.c_int * 3)()
        self._chk(self.lib.dav_comm_path(self.h, C.byref(sel), C.byref(ran), C.byref(cols), ms, valid))
        names = {-1: "undecided", 0: "program order", 1: "direct exchange", 2: "second stream"}
        return {"selected": names[sel.value], "trial_ran": bool(ran.value), "columns": cols.value,
                "trial_ms_max_over_ranks": {names[i]: round(ms[i], 4) for i in range(3)},
                "validated": {names[i]: bool(valid[i]) for i in range(3)}}

    def comm_init_shm(self, name: str):
        """Test transport for ranks that are processes sharing one GPU (POSIX shared memory `name`)."""
        self._chk(self.lib.dav_comm_init_shm(self.h, name.encode()))

    @staticmethod
    def comm_unique_id() -> bytes:
        lib = hip_lib()
        buf = C.create_string_buffer(128)
        if lib.dav_comm_unique_id(buf) != 0:
            raise DavidsonHipError(lib.dav_last_error().decode())
        return buf.raw

    # -- operators
    def device_memory(self):
        """(free, total) bytes of the engine's device"""
        f, t = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.dav_device_memory(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def set_storage(self, mode):
        """0 = full storage, 1 = symmetric-tiled (lower block triangle only)."""
        self._chk(self.lib.dav_set_storage(self.h, mode))

    def set_dense_host(self, which, a):
        a = _f(a)
        self._chk(self.lib.dav_set_dense_host(self.h, which, _dp(a), a.shape[0]))

    def set_dense_dev(self, which, dev_ptr, lda):
        """a(lda, n) column-major in device memory (e.g. a torch tensor's data_ptr())."""
        self._chk(self.lib.dav_set_dense_dev(self.h, which, dev_ptr, lda))

    def set_dense_generated(self, which, seed, sparsity, diag_val=None):
        self._chk(self.lib.dav_set_dense_generated(self.h, which, seed, sparsity, *_optional(diag_val)))

    # -- streaming ingest (rows in the reference's on-disk order, row-major)
    def dense_begin(self, which):
        self._chk(self.lib.dav_dense_begin(self.h, which))

    def dense_put_rows(self, which, row0, rows):
        """rows: (nrows, n) C-ordered block of complete rows, global rows row0..row0+nrows-1."""
        r = np.ascontiguousarray(rows, dtype=np.float64)
        self._chk(self.lib.dav_dense_put_rows(self.h, which, row0, r.shape[0], _dp(r), r.shape[1]))

    def dense_end(self, which):
        self._chk(self.lib.dav_dense_end(self.h, which))

    def set_dense_file(self, which, path, fmt="text"):
        """fmt: "text" = the reference's write_matrix/read_matrix format, "f64" = raw row-major float64."""
        code = {"text": 0, "f64": 1}[fmt]
        self._chk(self.lib.dav_set_dense_file(self.h, which, str(path).encode(), code))

    def set_operator_hashed(self, which, seed, sparsity, diag_val=None):
        self._chk(self.lib.dav_set_operator_hashed(self.h, which, seed, sparsity, *_optional(diag_val)))

    def set_operator_harness(self, which, e_table):
        e = np.ascontiguousarray(e_table, dtype=np.float64)
        self._chk(self.lib.dav_set_operator_harness(self.h, which, _dp(e)))

    def set_operator_identity(self, which):
        self._chk(self.lib.dav_set_operator_identity(self.h, which))

    def set_operator_host(self, which, diag):
        d = np.ascontiguousarray(diag, dtype=np.float64)
        self._chk(self.lib.dav_set_operator_host(self.h, which, _dp(d)))

    def set_operator_device(self, which, fn, ctx, diag):
        """The caller's own block apply on device memory (dav_device_apply_fn): `fn` a ctypes function pointer (DEVICE_APPLY_FN or a
        symbol of a loaded library), `ctx` an integer / c_void_p passed through, `diag` the operator's diagonal (n) - for which = OP_M it
        is not read and may be None."""
        if diag is None and which != OP_M:
            raise ValueError("set_operator_device: only the preconditioner (which = OP_M) goes without its diagonal")
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.float64)
        self._device_ops = getattr(self, "_device_ops", {})
        self._device_ops[which] = (fn, ctx)                # keep the callback alive as long as the engine
        self._chk(self.lib.dav_set_operator_device(self.h, which, fn, ctx, None if d is None else _dp(d)))

    def set_operator_csr(self, which, indptr, indices=None, data=None, base=0, lower=False, diagonals=False):
        """dav_set_operator_csr: a symmetric matrix in CSR form (the global arrays; indptr / indices numbered from `base`), every nonzero
        (lower=False) or only the entries with column <= row (lower=True).  Three numpy arrays, or one object with .tocsr(), or a
        torch.sparse_csr_tensor (one on the GPU goes to set_operator_csr_dev).  The engine validates the input (DavidsonHipError) and
        leaves the operator unset when it refuses it.  diagonals=True (DAV_CSR_DIAGONALS): the matrix is stored by its diagonals - for
        stencils and banded matrices; one with too many diagonals for its entries is refused, never stored as CSR instead."""
        if is_torch_csr(indptr):
            parts = torch_csr_parts(indptr)
            if indptr.device.type != "cpu":
                return self.set_operator_csr_dev(which, *parts, base=base, lower=lower, diagonals=diagonals)
            indptr, indices, data = parts
        rp, ci, vv = csr_arrays(indptr, indices, data, self.n)
        ci_p = ci.ctypes.data_as(C.POINTER(C.c_int32)) if ci.size else (C.c_int32 * 1)()
        vv_p = _dp(vv) if vv.size else (C.c_double * 1)()
        self._saw_values(which, None)
        self._chk(self.lib.dav_set_operator_csr(self.h, which, rp.ctypes.data_as(C.POINTER(C.c_int64)), ci_p, vv_p, base,
                                                csr_flag_word(lower, diagonals)))
        self._saw_values(which, int(rp[-1] - rp[0]))

    def set_operator_csr_dev(self, which, row_ptr, col_idx, vals, base=0, lower=False, diagonals=False):
        """dav_set_operator_csr_dev: the matrix of set_operator_csr as torch tensors on the engine's device, built on the GPU - row_ptr
        (n + 1) and col_idx int32 or int64, vals float64, all contiguous.  Other dtypes are a TypeError (never converted).  Torch's
        current stream on the device is synchronised first, so work queued on it that writes the arrays is complete.  The engine's
        refusal is a DavidsonHipError; the operator is then unset.  diagonals: as for set_operator_csr."""
        rpb, cib, nnz = _device_csr_tensors(row_ptr, col_idx, vals, self.n, self.device)
        import torch
        torch.cuda.current_stream(row_ptr.device).synchronize()
        self._saw_values(which, None)
        self._chk(self.lib.dav_set_operator_csr_dev(self.h, which, row_ptr.data_ptr(), rpb, col_idx.data_ptr() or None, cib,
                                                    vals.data_ptr() or None, base, csr_flag_word(lower, diagonals)))
        self._saw_values(which, nnz)

    def set_operator_coo(self, which, rows, cols=None, vals=None, base=0, lower=False, diagonals=False):
        """davx_set_operator_coo: the symmetric matrix of set_operator_csr as COO triples (rows[p], cols[p], vals[p]) in any order,
        duplicates included and kept as separate terms in the order of p - the operator is, bit for bit, that of the CSR matrix a
        stable sort of the triples by row gives.  Three numpy arrays, or a scipy coo_matrix (its .row, .col and .data as they stand:
        no sum_duplicates, no tocsr), or a torch.sparse_coo_tensor (its _indices() and _values() as they stand, coalesced or not; one
        on the GPU goes to set_operator_coo_dev).  The engine validates the input (DavidsonHipError names the first offending
        triple) and leaves the operator unset when it refuses it.  After keep_value_map, update_operator_values takes the values in
        the order of the triples.  lower, diagonals: as for set_operator_csr."""
        rows, cols, vals = coo_triples(rows, cols, vals)
        if type(vals).__module__.startswith("torch"):
            return self.set_operator_coo_dev(which, rows, cols, vals, base=base, lower=lower, diagonals=diagonals)
        ri, ci, vv = coo_arrays(rows, cols, vals)
        i32p = C.POINTER(C.c_int32)
        self._saw_values(which, None)
        self._chk(self.lib.davx_set_operator_coo(self.h, which, vv.size, ri.ctypes.data_as(i32p) if vv.size else None,
                                                ci.ctypes.data_as(i32p) if vv.size else None, _dp(vv) if vv.size else None, base,
                                                csr_flag_word(lower, diagonals)))
        self._saw_values(which, int(vv.size))

    def set_operator_coo_dev(self, which, rows, cols, vals, base=0, lower=False, diagonals=False):
        """davx_set_operator_coo_dev: the triples of set_operator_coo as torch tensors on the engine's device, bucketed by row and
        sorted on the GPU - rows and cols int32 or int64, vals float64, all contiguous and of one length.  Other dtypes are a TypeError
        (never converted).  Torch's current stream on the device is synchronised first.  The engine's refusal is a DavidsonHipError;
        the operator is then unset."""
        rb, cb, nnz = _device_coo_tensors(rows, cols, vals, self.device)
        import torch
        torch.cuda.current_stream(vals.device).synchronize()
        self._saw_values(which, None)
        self._chk(self.lib.davx_set_operator_coo_dev(self.h, which, nnz, rows.data_ptr() or None, rb, cols.data_ptr() or None, cb,
                                                    vals.data_ptr() or None, base, csr_flag_word(lower, diagonals)))
        self._saw_values(which, nnz)

    def set_operator_bsr(self, which, indptr, indices=None, data=None, base=0, lower=False, layout=BSR_ROW_MAJOR):
        """dav_set_operator_bsr: a symmetric matrix in BSR form with square blocks (the global arrays; indptr / indices count block
        rows / columns from `base`), every nonzero block (lower=False) or only the blocks with block column <= block row (lower=True).
        Three numpy arrays - data of shape (nnzb, b, b), row-major blocks unless layout=BSR_COL_MAJOR - or one object with .indptr,
        .indices, .data and .blocksize (a scipy bsr_matrix), or a torch.sparse_bsr_tensor (row-major blocks; one on the GPU goes to
        set_operator_bsr_dev).  The engine validates the input (DavidsonHipError) and leaves the operator unset when it refuses it."""
        if is_torch_bsr(indptr):
            parts = torch_bsr_parts(indptr)
            if indptr.device.type != "cpu":
                return self.set_operator_bsr_dev(which, *parts, base=base, lower=lower, layout=BSR_ROW_MAJOR)
            (indptr, indices, data), layout = parts, BSR_ROW_MAJOR
        b, rp, ci, vv = bsr_arrays(indptr, indices, data, self.n, layout)
        ci_p = ci.ctypes.data_as(C.POINTER(C.c_int32)) if ci.size else (C.c_int32 * 1)()
        vv_p = _dp(vv) if vv.size else (C.c_double * 1)()
        self._saw_values(which, None)
        self._chk(self.lib.dav_set_operator_bsr(self.h, which, b, rp.ctypes.data_as(C.POINTER(C.c_int64)), ci_p, vv_p, base,
                                                CSR_LOWER if lower else CSR_FULL, layout))
        self._saw_values(which, int(rp[-1] - rp[0]) * b * b)

    def set_operator_bsr_dev(self, which, row_ptr, col_idx, vals, base=0, lower=False, layout=BSR_ROW_MAJOR):
        """dav_set_operator_bsr_dev: the matrix of set_operator_bsr as torch tensors on the engine's device, built on the GPU - row_ptr
        (n / b + 1) and col_idx int32 or int64, vals float64 of shape (nnzb, b, b), all contiguous.  Other dtypes are a TypeError (never
        converted).  Torch's current stream on the device is synchronised first, so work queued on it that writes the arrays is
        complete.  The engine's refusal is a DavidsonHipError; the operator is then unset."""
        b, rpb, cib, nnzb = _device_bsr_tensors(row_ptr, col_idx, vals, self.n, self.device)
        import torch
        torch.cuda.current_stream(row_ptr.device).synchronize()
        self._saw_values(which, None)
        self._chk(self.lib.dav_set_operator_bsr_dev(self.h, which, b, row_ptr.data_ptr(), rpb, col_idx.data_ptr() or None, cib,
                                                    vals.data_ptr() or None, base, CSR_LOWER if lower else CSR_FULL, layout))
        self._saw_values(which, nnzb * b * b)

    def set_operator_csr_hermitian(self, which, indptr, indices=None, data=None, base=0, lower=False):
        """davh_set_operator_csr: a complex Hermitian matrix of order n / 2 in CSR form on this engine of the real order n, through its
        real form - every entry a + ib the block [[a, -b], [b, a]] of a BSR operator with block size 2 (include/davidson_hip_herm.h).
        Three arrays with data complex128, a scipy csr_matrix of complex dtype or a complex torch.sparse_csr_tensor (one on the GPU goes
        to set_operator_csr_hermitian_dev); the complex values are read where they lie.  lower=True: only the entries with column <= row
        are given; the strict lower ones are mirrored as conjugates.  The engine validates the input (DavidsonHipError; a diagonal entry
        with an imaginary part is refused) and leaves the operator unset when it refuses it.  After keep_value_map,
        update_operator_values takes complex128 values in the order of this call."""
        if is_torch_csr(indptr) and indptr.device.type != "cpu":
            return self.set_operator_csr_hermitian_dev(which, *torch_csr_parts(indptr), base=base, lower=lower)
        rp, ci, vv = hermitian_arrays(indptr, indices, data, self.n // 2 if self.n % 2 == 0 else None)
        ci_p = ci.ctypes.data_as(C.POINTER(C.c_int32)) if ci.size else (C.c_int32 * 1)()
        vv_p = vv.ctypes.data_as(C.c_void_p) if vv.size else (C.c_double * 2)()
        self._saw_values(which, None)
        self._chk(self.lib.davh_set_operator_csr(self.h, which, rp.ctypes.data_as(C.POINTER(C.c_int64)), ci_p, vv_p, base,
                                                 CSR_LOWER if lower else CSR_FULL))
        self._saw_values(which, int(rp[-1] - rp[0]), pairs=True)

    def set_operator_csr_hermitian_dev(self, which, row_ptr, col_idx, vals, base=0, lower=False):
        """davh_set_operator_csr_dev: the matrix of set_operator_csr_hermitian as torch tensors on the engine's device, built on the
        GPU - row_ptr (n / 2 + 1) and col_idx int32 or int64, vals complex128, all contiguous.  Other dtypes are a TypeError (never
        converted).  Torch's current stream on the device is synchronised first.  The engine's refusal is a DavidsonHipError; the
        operator is then unset."""
        if self.n % 2:
            raise DavidsonHipError(f"set_operator_csr_hermitian_dev: the engine's order {self.n} is odd; a Hermitian operator of order "
                                   "n / 2 needs an engine of the even real order n")
        rpb, cib, nnz = _device_hermitian_tensors(row_ptr, col_idx, vals, self.n // 2, self.device)
        import torch
        torch.cuda.current_stream(row_ptr.device).synchronize()
        self._saw_values(which, None)
        self._chk(self.lib.davh_set_operator_csr_dev(self.h, which, row_ptr.data_ptr(), rpb, col_idx.data_ptr() or None, cib,
                                                     vals.data_ptr() or None, base, CSR_LOWER if lower else CSR_FULL))
        self._saw_values(which, nnz, pairs=True)

    def build_fsai(self, sigma=0.0, level=1):
        """davp_build_fsai: the factorized sparse approximate inverse M = G^T G of A - sigma B on the pattern of tril(A)^level, level 1..3,
        into slot OP_M (include/davidson_hip_precond.h has the definition).  A is the CSR operator of slot OP_A, B a CSR operator or the
        identity, A - sigma B positive definite, one rank.  The engine's refusal is a DavidsonHipError; slot OP_M is then unset."""
        self._saw_values(OP_M, None)
        self._chk(self.lib.davp_build_fsai(self.h, float(sigma), int(level)))

    def fsai_info(self):
        """davp_fsai_info: (entries of G, longest row of G, longest row of G^T); zeros when slot OP_M holds no built preconditioner"""
        nnz, row, col = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.davp_fsai_info(self.h, C.byref(nnz), C.byref(row), C.byref(col)))
        return nnz.value, row.value, col.value

    def fsai_factor(self, transposed=False):
        """davp_fsai_get_factor: (indptr int64, indices int32, data float64) of G - transposed=True: of the store of G^T - as 0-based
        CSR numpy arrays"""
        nnz = self.fsai_info()[0]
        rp = np.zeros(self.n + 1, dtype=np.int64)
        ci = np.zeros(max(nnz, 1), dtype=np.int32)
        vv = np.zeros(max(nnz, 1), dtype=np.float64)
        self._chk(self.lib.davp_fsai_get_factor(self.h, int(bool(transposed)), rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                                _dp(vv)))
        return rp, ci[:nnz], vv[:nnz]

    def build_block_fsai(self, sigma=0.0, level=1):
        """davq_build_block_fsai: the block factorized sparse approximate inverse M = G^T G of A - sigma B on the pattern of tril(A)^level
        over the block index arrays, level 1..3, into slot OP_M (include/davidson_hip_bprecond.h has the definition).  A is the BSR
        operator of slot OP_A (a Hermitian operator is one, b = 2), B a BSR operator of the same block size or the identity, A - sigma B
        positive definite, one rank.  The engine's refusal is a DavidsonHipError; slot OP_M is then unset."""
        self._saw_values(OP_M, None)
        self._chk(self.lib.davq_build_block_fsai(self.h, float(sigma), int(level)))

    def block_fsai_info(self):
        """davq_block_fsai_info: (block size, blocks of G, longest block row of G, longest block row of G^T); zeros when slot OP_M
        holds no built block preconditioner"""
        b, nnzb, row, col = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.davq_block_fsai_info(self.h, C.byref(b), C.byref(nnzb), C.byref(row), C.byref(col)))
        return b.value, nnzb.value, row.value, col.value

    def block_fsai_factor(self, transposed=False):
        """davq_block_fsai_get_factor: (indptr int64, indices int32, data float64 (nnzb, b, b) row-major blocks) of G - transposed=True:
        of the store of G^T - as 0-based BSR numpy arrays, as set_operator_bsr takes them"""
        b, nnzb = self.block_fsai_info()[:2]
        if b == 0:
            self._chk(self.lib.davq_block_fsai_get_factor(self.h, int(bool(transposed)), None, None, None))
        rp = np.zeros(self.n // b + 1, dtype=np.int64)
        ci = np.zeros(max(nnzb, 1), dtype=np.int32)
        vv = np.zeros((max(nnzb, 1), b, b), dtype=np.float64)
        self._chk(self.lib.davq_block_fsai_get_factor(self.h, int(bool(transposed)), rp.ctypes.data_as(C.c_void_p),
                                                      ci.ctypes.data_as(C.c_void_p), _dp(vv)))
        return rp, ci[:nnzb], vv[:nnzb]

    def _saw_values(self, which, count, pairs=False):
        """the number of values the sparse set call of operator `which` saw (None: unknown - a refused call, or one not made here);
        pairs: they are complex (re, im) pairs (set_operator_csr_hermitian)"""
        self._value_counts = getattr(self, "_value_counts", {})
        self._value_counts[which] = count
        self._value_pairs = getattr(self, "_value_pairs", {})
        self._value_pairs[which] = pairs

    def keep_value_map(self, which, on=True):
        """dav_keep_value_map: a sticky switch per operator; the NEXT sparse set call of `which` also keeps where every stored value came
        from (8 bytes per entry or block of this rank, 16 per row or block row), which update_operator_values needs.  No effect on an
        operator that is already set."""
        self._chk(self.lib.dav_keep_value_map(self.h, which, int(on)))

    def update_operator_values(self, which, vals):
        """dav_update_operator_values / dav_update_operator_values_dev: new values on the kept pattern of a CSR or BSR operator set after
        keep_value_map(which) - `vals` as long and in the order (BSR: block layout; (nnzb, b, b) or flat) of the vals of that set call.
        A numpy array (or a torch tensor on the CPU) goes through the host entry; a torch tensor on the engine's device through the
        device entry, after torch's current stream on the device has been synchronised.  float64 only - complex128 only for an operator
        set by set_operator_csr_hermitian, one value per entry - (TypeError, never converted); a
        length other than what the set call saw is a ValueError before the engine is called.  The engine's refusal - no value map, not
        a sparse operator - is a DavidsonHipError, and the operator keeps its old values."""
        host, dev = update_values_array(vals, getattr(self, "_value_counts", {}).get(which), self.device,
                                        pairs=getattr(self, "_value_pairs", {}).get(which, False))
        if dev is not None:
            import torch
            torch.cuda.current_stream(dev.device).synchronize()
            self._chk(self.lib.dav_update_operator_values_dev(self.h, which, dev.data_ptr() or None))
        else:
            self._chk(self.lib.dav_update_operator_values(self.h, which, host.ctypes.data_as(C.c_void_p) if host.size else (C.c_double * 2)()))

    def get_diagonal(self, which):
        d = np.zeros(self.n)
        self._chk(self.lib.dav_get_diagonal(self.h, which, _dp(d)))
        return d

    # -- hot path
    def init_basis(self, ncols):
        idx = np.zeros(ncols, dtype=np.int64)
        self._chk(self.lib.dav_init_basis(self.h, ncols, idx.ctypes.data_as(C.POINTER(C.c_int64))))
        return idx

    # -- warm start
    def set_guess(self, x):
        """dav_set_guess / dav_set_guess_dev: the columns of x (n rows) become the staged guess of the next solve.  A numpy array (or a
        torch tensor on the CPU) goes through the host entry; a torch tensor on the engine's device through the device entry, after
        torch's current stream on the device has been synchronised.  float64 only (TypeError, never converted); a wrong row count is a
        ValueError before the engine is called.  The engine's refusal - too many columns, an entry that is not finite, a column that is
        entirely zero - is a DavidsonHipError, and a guess staged earlier stays staged."""
        host, dev = guess_array(x, self.n, self.device)
        if dev is not None:
            import torch
            t, ld, ncols = dev
            torch.cuda.current_stream(t.device).synchronize()
            self._chk(self.lib.dav_set_guess_dev(self.h, t.data_ptr() or None, ld, ncols))
        else:
            self._chk(self.lib.dav_set_guess(self.h, _dp(host), host.shape[0], host.shape[1]))

    def set_guess_raw(self, x, ldx, ncols):
        """dav_set_guess with an explicit leading dimension: x a one-dimensional float64 array holding x(ldx, ncols) column-major"""
        a = np.ascontiguousarray(x, dtype=np.float64)
        self._chk(self.lib.dav_set_guess(self.h, _dp(a), ldx, ncols))

    def set_guess_dev_raw(self, dev_ptr, ldx, ncols):
        """dav_set_guess_dev with a raw device pointer (e.g. a torch tensor's data_ptr() plus an offset) and leading dimension"""
        self._chk(self.lib.dav_set_guess_dev(self.h, dev_ptr, ldx, ncols))

    def keep_result_as_guess(self, on=True):
        """dav_keep_result_as_guess: sticky; while on, the Ritz vectors a solve leaves in X are the staged guess of the next solve"""
        self._chk(self.lib.dav_keep_result_as_guess(self.h, int(on)))

    def guess_columns(self):
        """dav_guess_columns: staged guess columns, 0 = none"""
        g = C.c_int(0)
        self._chk(self.lib.dav_guess_columns(self.h, C.byref(g)))
        return g.value

    def init_basis_guess(self, ncols):
        """dav_init_basis_guess: (idx, g) - the staged columns in V[:, 0:g), unit vectors behind them (idx: 0 for a guess column, the
        1-based position for a unit column); no images: orthonormalise, then expand(0, ncols) and project(0, ncols)"""
        idx = np.zeros(ncols, dtype=np.int64)
        g = C.c_int(0)
        self._chk(self.lib.dav_init_basis_guess(self.h, ncols, idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(g)))
        return idx, g.value

    def apply(self, which, src_panel, c0, k, dst_panel, d0):
        self._chk(self.lib.dav_apply(self.h, which, src_panel, c0, k, dst_panel, d0))

    def apply_inner(self, which, src_panel, c0, k, dst_panel, d0):
        """dav_apply as the GJD correction solve issues it (may read the fp32 copy of the tiles; csrc/davidson_hip_private.h)"""
        self._chk(self.lib.dav_apply_inner(self.h, which, src_panel, c0, k, dst_panel, d0))

    def resident_fraction(self, which):
        f = C.c_double()
        self._chk(self.lib.dav_resident_fraction(self.h, which, C.byref(f)))
        return f.value

    def gram(self, panel_p, p0, p, panel_q, q0, q):
        out = np.zeros((p, q), order="F")
        self._chk(self.lib.dav_gram(self.h, panel_p, p0, p, panel_q, q0, q, _dp(out), p))
        return out

    def project(self, c0, k, H, S=None):
        ld = H.shape[0]
        sp = _dp(S) if S is not None else C.POINTER(C.c_double)()
        self._chk(self.lib.dav_project(self.h, c0, k, _dp(H), ld, sp, ld))

    def ritz_residual_correction(self, m, lowest, Y, theta, method=METHOD_DPR):
        Y = _f(Y)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        res = np.zeros(lowest)
        self._chk(self.lib.dav_ritz_residual_correction(self.h, m, lowest, _dp(Y), Y.shape[0], _dp(theta), method, _dp(res)))
        return res

    def ritz_residual_correction_n(self, m, ncorr, lowest, Y, theta, method=METHOD_DPR):
        """dav_ritz_residual_correction_n: corrections / residues for the first ncorr Ritz pairs, norms of the first `lowest`"""
        Y = _f(Y)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        res = np.zeros(lowest)
        self._chk(self.lib.dav_ritz_residual_correction_n(self.h, m, ncorr, lowest, _dp(Y), Y.shape[0], _dp(theta), method, _dp(res)))
        return res

    def ritz_residual_correction_g(self, m, ncorr, lowest, Y, theta):
        """dav_ritz_residual_correction_g: the DPR phase with (resnorm, C = V^T T, G = T^T T) of the new block in the same fetch"""
        Y = _f(Y)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        res = np.zeros(lowest)
        Cm, G = np.zeros((m, ncorr), order="F"), np.zeros((ncorr, ncorr), order="F")
        self._chk(self.lib.dav_ritz_residual_correction_g(self.h, m, ncorr, lowest, _dp(Y), Y.shape[0], _dp(theta), _dp(res), _dp(Cm), m,
                                                          _dp(G), ncorr))
        return res, Cm, G

    def set_lazy_ritz_vectors(self, on=True):
        """dav_set_lazy_ritz_vectors: while on, the Ritz phases write X only for GJD; ritz_vectors makes it on demand"""
        self._chk(self.lib.dav_set_lazy_ritz_vectors(self.h, int(on)))

    def ritz_vectors(self, m, nx, Y):
        """dav_ritz_vectors: X[:, :nx] = V[:, :m] Y[:, :nx]"""
        Y = _f(Y)
        self._chk(self.lib.dav_ritz_vectors(self.h, m, nx, _dp(Y), Y.shape[0]))

    def panel_select(self, panel, c0, sel):
        """dav_panel_select: column c0 + i of the panel <- column c0 + sel[i] (ascending indices, sel[i] >= i)"""
        s = np.ascontiguousarray(sel, dtype=np.int32)
        self._chk(self.lib.dav_panel_select(self.h, panel, c0, s.size, s.ctypes.data_as(C.POINTER(C.c_int))))

    def gjd_correction_steps(self, mbasis, ncols, theta, steps):
        """dav_gjd_correction_n with inner_tol = 0 and no per-column tolerances: every column that starts takes `steps` inner steps
        (unless it breaks down).  T lands in V[:, mbasis:mbasis + ncols]; returns the steps taken."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        assert theta.size >= ncols
        it = C.c_int(-1)
        self._chk(self.lib.dav_gjd_correction_n(self.h, mbasis, ncols, _dp(theta), steps, 0.0, None, C.byref(it)))
        return it.value

    def gjd_correction(self, m, theta, max_inner=500, inner_tol=1e-12):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        it = C.c_int(0)
        self._chk(self.lib.dav_gjd_correction(self.h, m, _dp(theta), max_inner, inner_tol, C.byref(it)))
        return it.value

    def gjd_correction_n(self, m, ncols, theta, tol_per_col, max_inner=500, inner_tol=1e-12):
        """dav_gjd_correction_n: per-column relative tolerances; a negative entry marks a follower (stops at |tol| or when every
        column with a positive entry has stopped)"""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        tols = np.ascontiguousarray(tol_per_col, dtype=np.float64)
        assert theta.size >= ncols and tols.size >= ncols
        it = C.c_int(0)
        self._chk(self.lib.dav_gjd_correction_n(self.h, m, ncols, _dp(theta), max_inner, inner_tol, _dp(tols), C.byref(it)))
        return it.value

    def ortho_gram(self, m, kt):
        Cm = np.zeros((max(m, 1), kt), order="F")
        G = np.zeros((kt, kt), order="F")
        self._chk(self.lib.dav_ortho_gram(self.h, m, kt, _dp(Cm), max(m, 1), _dp(G), kt))
        return Cm[:m], G

    def ortho_apply(self, m, kt, Cm, M):
        Cm = _f(Cm) if m > 0 else np.zeros((1, kt), order="F")
        M = _f(M)
        self._chk(self.lib.dav_ortho_apply(self.h, m, kt, _dp(Cm), Cm.shape[0], _dp(M), M.shape[0]))

    def ortho_apply_all(self, m, kt, Cm, M):
        """dav_ortho_apply on T and on its images in the W (and BV) panels"""
        Cm = _f(Cm) if m > 0 else np.zeros((1, kt), order="F")
        M = _f(M)
        self._chk(self.lib.dav_ortho_apply_all(self.h, m, kt, _dp(Cm), Cm.shape[0], _dp(M), M.shape[0]))

    def project_ortho(self, m, k, gev=False):
        """dav_project_ortho: ([V T]^T (A T), [V T]^T (B T) | None, V^T T, T^T T) in one fetch"""
        p = m + k
        H = np.zeros((p, k), order="F")
        S = np.zeros((p, k), order="F") if gev else None
        Cm = np.zeros((max(m, 1), k), order="F")
        G = np.zeros((k, k), order="F")
        sp = _dp(S) if gev else C.POINTER(C.c_double)()
        self._chk(self.lib.dav_project_ortho(self.h, m, k, _dp(H), p, sp, p, _dp(Cm), max(m, 1), _dp(G), k))
        return H, S, Cm[:m], G

    def expand(self, m, kt):
        self._chk(self.lib.dav_expand(self.h, m, kt))

    def restart(self, m, keep, Yk):
        Yk = _f(Yk)
        self._chk(self.lib.dav_restart(self.h, m, keep, _dp(Yk), Yk.shape[0]))

    def panel_transform(self, src_panel, s0, p, M, dst_panel, d0):
        M = _f(M)
        self._chk(self.lib.dav_panel_transform(self.h, src_panel, s0, p, _dp(M), M.shape[0], M.shape[1], dst_panel, d0))

    def panel_get(self, panel, c0, k):
        out = np.zeros((self.n, k), order="F")
        self._chk(self.lib.dav_panel_get(self.h, panel, c0, k, _dp(out), self.n))
        return out

    def panel_put(self, panel, c0, data):
        data = _f(data)
        self._chk(self.lib.dav_panel_put(self.h, panel, c0, data.shape[1], _dp(data), data.shape[0]))

    def set_width(self, m):
        self._chk(self.lib.dav_set_width(self.h, m))

    def ranks_agree(self, words):
        w = np.ascontiguousarray(words, dtype=np.float64)
        self._chk(self.lib.dav_ranks_agree(self.h, _dp(w), w.size))

    def agree_inputs(self, words):
        """the inputs of a solve, verified across the ranks in a fixed-size collective whenever they differ from the last verified ones"""
        w = np.ascontiguousarray(words, dtype=np.float64)
        self._chk(self.lib.dav_agree_inputs(self.h, _dp(w), w.size))

    def agree_next(self, words):
        w = np.ascontiguousarray(words, dtype=np.float64)
        self._chk(self.lib.dav_agree_next(self.h, _dp(w), w.size))

    def set_inner_precision(self, bits):
        self._chk(self.lib.dav_set_inner_precision(self.h, bits))

    def rr_enable(self, on=True):
        self._chk(self.lib.dav_rr_enable(self.h, int(on)))

    def project_dev(self, c0, k):
        self._chk(self.lib.dav_project_dev(self.h, c0, k))

    def rr_ritz(self, m, ncorr, lowest, method=METHOD_DPR, want_gram=False):
        """(theta[m], resnorm[lowest], sweeps[, C, G]) from the device-resident projected matrices"""
        theta, res, sweeps = np.zeros(m), np.zeros(lowest), C.c_int(0)
        if want_gram:
            Cm, G = np.zeros((m, ncorr), order="F"), np.zeros((ncorr, ncorr), order="F")
            self._chk(self.lib.dav_rr_ritz(self.h, m, ncorr, lowest, method, _dp(theta), _dp(res), _dp(Cm), m, _dp(G), ncorr,
                                           C.byref(sweeps)))
            return theta, res, sweeps.value, Cm, G
        self._chk(self.lib.dav_rr_ritz(self.h, m, ncorr, lowest, method, _dp(theta), _dp(res), None, 0, None, 0, C.byref(sweeps)))
        return theta, res, sweeps.value

    def rr_restart(self, m, keep):
        """collapse restart with the device-resident eigenvectors: V, W (and B V) <- their first `keep` Ritz combinations"""
        self._chk(self.lib.dav_rr_restart(self.h, m, keep))

    def rr_get(self, m, ncols):
        theta, Y = np.zeros(m), np.zeros((m, ncols), order="F")
        self._chk(self.lib.dav_rr_get(self.h, m, ncols, _dp(theta), _dp(Y), m))
        return theta, Y

    def bench_apply(self, k, reps, which=OP_A):
        """(ms per apply END TO END: pack + kernel + reduction, algorithmic bytes per apply)"""
        ms, nbytes = C.c_double(), C.c_double()
        self._chk(self.lib.dav_bench_apply(self.h, which, k, reps, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def bench_stream(self, doubles=0, reps=5):
        """(copy GB/s, triad GB/s) of plain streaming kernels on this box (read + written bytes)"""
        cp, tr = C.c_double(), C.c_double()
        self._chk(self.lib.dav_bench_stream(self.h, doubles, reps, C.byref(cp), C.byref(tr)))
        return cp.value, tr.value

    def bench_stream3(self, doubles=0, reps=5):
        """(copy, triad, read-only GB/s): bench_stream plus a kernel that only reads (two arrays, one partial sum per workgroup written)"""
        cp, tr, rd = C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.dav_bench_stream3(self.h, doubles, reps, C.byref(cp), C.byref(tr), C.byref(rd)))
        return cp.value, tr.value, rd.value

    def bench_harness_rate(self, iters=2000):
        """entries per second of the matrix-free test operator's arithmetic (atan2 + sqrt + log + cos, fp64) on registers"""
        r = C.c_double(0.0)
        self._chk(self.lib.dav_bench_harness_rate(self.h, iters, C.byref(r)))
        return r.value

    def bench_apply2(self, k, reps, which=OP_A):
        """(ms per apply end to end, ms of the block-matvec kernel alone, algorithmic bytes, flops) per apply"""
        ms, kms, nbytes, flops = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.dav_bench_apply2(self.h, which, k, reps, C.byref(ms), C.byref(kms), C.byref(nbytes), C.byref(flops)))
        return ms.value, kms.value, nbytes.value, flops.value


def parse_text_f64(data: bytes) -> np.ndarray:
    """The engine's parser of the reference's text dumps (host only): all numbers in `data`."""
    lib = hip_lib()
    n = C.c_size_t(0)
    if lib.dav_parse_text_f64(data, len(data), None, 0, C.byref(n)) != 0:
        raise DavidsonHipError(lib.dav_last_error().decode())
    out = np.empty(n.value)
    if lib.dav_parse_text_f64(data, len(data), _dp(out), out.size, C.byref(n)) != 0:
        raise DavidsonHipError(lib.dav_last_error().decode())
    return out


def buffer_cache_held():
    """(idle device bytes, idle pinned host bytes) the buffer cache holds right now (measurement door, csrc/davidson_hip_private.h)"""
    lib = hip_lib()
    d, h = C.c_int64(), C.c_int64()
    lib.dav_buffer_cache_held(C.byref(d), C.byref(h))
    return d.value, h.value


def free_buffers() -> None:
    """Return the buffer cache's idle device / pinned blocks (kept from the engine destroyed last) to the device."""
    hip_lib().dav_free_buffers()
