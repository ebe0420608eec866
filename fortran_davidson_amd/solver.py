"""Python mirror of the reference's Fortran interface, forwarding to the Fortran host library.

    generalized_eigensolver(matrix | callable, lowest, method, max_iterations, tolerance,
                            max_dim_sub=None, second_matrix | callable=None)
        -> (eigenvalues, eigenvectors, iters)

mirrors `call generalized_eigensolver(mtx, eigenvalues, eigenvectors, lowest, method, max_iterations,
tolerance, iters [, max_dim_sub] [, second_matrix])` of module davidson (reference:
src/davidson.f90:51-52, :277-278), outputs returned instead of passed.  Every call goes
Python -> libfortran_davidson_amd.so (Fortran driver loop) -> libdavidson_hip.so (HIP kernels).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import fortran_lib, hip_lib
from .engine_c import (CEngine, DavidsonHipError, _device_bsr_tensors, _device_coo_tensors, _device_csr_tensors, _device_hermitian_tensors,
                       _dp, _f, _optional, check_bsr, check_coo, check_csr, check_hermitian, coo_triples, csr_flag_word, device_bsr_tensors, device_csr_tensors, guess_array, is_torch_bsr,
                       is_torch_coo, is_torch_csr, torch_bsr_parts, torch_csr_parts, update_values_array)

# The operator slots of DavidsonEngine, numbered as the Fortran routines number them.  OP_M is the caller's preconditioner - an
# approximation of (A - sigma B)^-1, symmetric, for "GJD" positive definite - which "DPR" (T = M R) and "GJD" (its MINRES) apply in place
# of the diagonal; "BDPR", "CHEB" and "LCHEB" do not read it.  It is set by set_sparse, set_block_sparse, set_device_operator and
# set_identity, refreshed by update_values, replaced by setting it again and never unset.  The one-shot functions of this module
# (generalized_eigensolver_sparse, generalized_eigensolver_bsr and the others) take no preconditioner: their doors have fixed argument lists.
OP_A, OP_B, OP_M = 1, 2, 3

_METHOD = {"DPR": 0, "GJD": 1, "BDPR": 3}
_DEGREE_METHOD = {"CHEB": 4, "LCHEB": 5}        # "<name>" (default degree) or "<name><d>" with 1 <= d <= 64: the degree rides in bits 8..15


def _parse_method(method):
    """(kind, degree) of a method name: _METHOD's and _DEGREE_METHOD's codes (engine_c.METHOD_*), degree 0 = none given (the engine's
    default); anything that is no method name: (2, 0) - the Fortran doors stop the process on a name they do not know.  ValueError: a
    degree outside 1..64."""
    for name in ("LCHEB", "CHEB"):
        if isinstance(method, str) and method.startswith(name):
            tail = method[len(name):]
            if tail == "":
                return _DEGREE_METHOD[name], 0
            if not (tail.isascii() and tail.isdigit()) or not 1 <= int(tail) <= 64:
                raise ValueError(f"method {method!r}: the degree of the Chebyshev correction is {name!r} (default) or '{name}<d>' with "
                                 "1 <= d <= 64")
            return _DEGREE_METHOD[name], int(tail)
    return _METHOD.get(method, 2), 0


def _method_code(method):
    """the integer the doors take (engine_c.method_code): kind | degree << 8; unknown names: 2"""
    kind, degree = _parse_method(method)
    return kind | degree << 8


def _check_method(method, *, a_sparse=False, blocks=None, gev=False, host_callbacks=False, n=0, nranks=1,
                  where="generalized_eigensolver"):
    """What a method does not serve, refused here (ValueError) before any engine call: the engine refuses it at the first correction and
    the Fortran doors stop the process on an engine error.
    "BDPR" (block-diagonal DPR) serves BSR operators only - A of any block size 1..16, B (generalized problems) of the same one, and
    with several ranks a block size that divides the rows of a rank's slab.  blocks: the block sizes of A and B as the caller set them,
    None = not a BSR operator; blocks=None: a front end that learns them only from its input leaves the check to the engine.
    "CHEB" / "CHEB<d>" (Chebyshev-filtered correction) serves standard problems whose operator A is a CSR or BSR operator (a_sparse): its
    spectral bound comes from the stored entries.
    "LCHEB" / "LCHEB<d>" (the same correction with a Lanczos bound) serves standard problems whose operator A the engine applies on the
    device - every kind but a host callback."""
    kind, _ = _parse_method(method)
    if kind == 3 and blocks is not None:
        ba, bb = blocks
        if ba is None:
            raise ValueError(f"{where}: method 'BDPR' needs operator A in BSR form (generalized_eigensolver_bsr, "
                             "DavidsonEngine.set_block_sparse)")
        if gev and bb != ba:
            raise ValueError(f"{where}: method 'BDPR' needs operator B in BSR form with the block size of A ({ba}), not "
                             + ("another kind of operator" if bb is None else f"block size {bb}"))
        if nranks > 1:
            nslab = -(-(-(-n // nranks)) // 16) * 16
            if nslab % ba != 0:
                raise ValueError(f"{where}: method 'BDPR' on {nranks} ranks needs a block size that divides the {nslab} rows of a rank's "
                                 f"slab, not {ba}")
    if kind == 4 and not a_sparse:
        raise ValueError(f"{where}: method {method!r} needs operator A in CSR or BSR form (generalized_eigensolver_sparse, "
                         "generalized_eigensolver_bsr, DavidsonEngine.set_sparse / set_block_sparse)")
    if kind == 5 and host_callbacks:
        raise ValueError(f"{where}: method {method!r} needs an operator A the engine applies on the device; host callbacks are not "
                         "served (DavidsonEngine.set_device_operator takes a device callback)")
    if kind in (4, 5) and gev:
        raise ValueError(f"{where}: method {method!r} serves standard problems only (the filter of a generalized problem would need "
                         "the inverse of B)")


def _check_bdpr(method, blocks, gev=False, n=0, nranks=1, where="generalized_eigensolver"):
    """_check_method for "BDPR" alone"""
    if method == "BDPR":
        _check_method(method, blocks=blocks, gev=gev, n=n, nranks=nranks, where=where)


def _check_cheb(method, sparse_a, gev=False, where="generalized_eigensolver"):
    """_check_method for "CHEB" / "CHEB<d>" alone"""
    if isinstance(method, str) and method.startswith("CHEB"):
        _check_method(method, a_sparse=sparse_a, gev=gev, where=where)


def _check_lcheb(method, gev=False, host_callbacks=False, where="generalized_eigensolver"):
    """_check_method for "LCHEB" / "LCHEB<d>" alone"""
    if isinstance(method, str) and method.startswith("LCHEB"):
        _check_method(method, gev=gev, host_callbacks=host_callbacks, where=where)


_CB = C.CFUNCTYPE(None, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))


def _initial_vectors(x, n, lowest):
    """initial_vectors= of the one-call front ends, checked here because their Fortran doors stop the process on a refused guess:
    float64 (TypeError), n rows, finite entries, no column that is entirely zero (ValueError).  Of a guess wider than the start basis
    (2 * lowest columns) the leading columns are used.  Returns a Fortran-ordered host array."""
    host, dev = guess_array(x, n, None, "initial_vectors")
    if dev is not None:
        host = np.asfortranarray(dev[0].cpu().numpy())
    host = np.asfortranarray(host[:, :2 * lowest])
    if not np.isfinite(host).all():
        raise ValueError("initial_vectors: x holds an entry that is not finite (Inf or NaN)")
    zero = np.flatnonzero(~(host != 0.0).any(axis=0))
    if zero.size:
        raise ValueError(f"initial_vectors: column {int(zero[0])} of x (counted from 0) is entirely zero")
    return host


def generalized_eigensolver(matrix, lowest, method, max_iterations, tolerance, max_dim_sub=None,
                            second_matrix=None, initial_vectors=None):
    """initial_vectors (n, g): the solve starts from these columns instead of unit vectors (Fortran: initial_vectors=)."""
    _check_method(method, blocks=(None, None), gev=second_matrix is not None)
    lib = fortran_lib()
    iters = C.c_int(-1)
    evals = np.zeros(lowest)
    if callable(matrix):
        # matrix-free specific: first argument is the block-apply callback; `second_matrix` is the
        # (mandatory, src/davidson.f90:366,379) B callback; the eigenvector array fixes n.
        raise TypeError("matrix-free call needs n: use generalized_eigensolver_free(fun_A, n, ...)")
    a = _f(matrix)
    n = a.shape[0]
    evecs = np.zeros((n, lowest), order="F")
    b = _f(second_matrix) if second_matrix is not None else np.zeros((1, 1), order="F")
    if initial_vectors is not None:
        x0 = _initial_vectors(initial_vectors, n, lowest)
        lib.fd_dense_solve_guess(n, _dp(a), int(second_matrix is not None), _dp(b), lowest, _method_code(method), max_iterations,
                                 tolerance, -1 if max_dim_sub is None else max_dim_sub, x0.shape[1], _dp(x0), _dp(evals), _dp(evecs),
                                 C.byref(iters))
        return evals, evecs, iters.value
    lib.fd_dense_solve(n, _dp(a), int(second_matrix is not None), _dp(b), lowest, _method_code(method), max_iterations, tolerance,
                       -1 if max_dim_sub is None else max_dim_sub, _dp(evals), _dp(evecs), C.byref(iters))
    return evals, evecs, iters.value


def _i64(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else (C.c_int32 * 1)()


def _sparse_input(a, n=None, lower=False):
    """(n, indptr, indices, data) of a CSR operator given as a tuple (indptr, indices, data) or an object with .tocsr(), 0-based,
    validated here (ValueError) - the Fortran door stops the process on an engine error"""
    if is_torch_csr(a):
        a = torch_csr_parts(a)
    if hasattr(a, "tocsr"):
        m = a.tocsr()
        a = (m.indptr, m.indices, m.data)
    indptr, indices, data = a
    n = len(indptr) - 1 if n is None else n
    rp, ci, vv = check_csr(indptr, indices, data, n, 0, lower)
    return n, rp, ci, vv if vv.size else np.zeros(1)


def _is_device_csr(a):
    return is_torch_csr(a) and a.device.type != "cpu"


def generalized_eigensolver_sparse(indptr, indices, data, lowest, method, max_iterations, tolerance, max_dim_sub=None, second=None,
                                   lower=False, initial_vectors=None, diagonals=False):
    """`call generalized_eigensolver(a_csr, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters [, max_dim_sub]
    [, b_csr])` (the csr_matrix specific of module davidson) with A in CSR form, 0-based: three arrays, or `indptr` an object with
    .tocsr() and indices = data = None.  `second`: B the same way - a tuple (indptr, indices, data) or an object with .tocsr().  Either
    may also be a torch.sparse_csr_tensor; one on the GPU is built there (DavidsonEngine.set_sparse on the tensor's device).
    lower=True: only the entries with column <= row are given, for A and B.  initial_vectors (n, g): the solve starts from these
    columns instead of unit vectors.  diagonals=True: A and B are stored by their diagonals (csr_matrix(..., diagonals=.true.); a
    matrix that does not suit the storage is refused).  Returns (eigenvalues, eigenvectors, iters)."""
    _check_method(method, a_sparse=True, blocks=(None, None), gev=second is not None, where="generalized_eigensolver_sparse")
    a = indptr if indices is None and data is None else (indptr, indices, data)
    if is_torch_coo(a) or is_torch_coo(second):
        # a torch.sparse_coo_tensor goes to the COO path as it stands (set_sparse routes each operator by its layout)
        first = a if is_torch_coo(a) else second
        n = a.shape[0] if hasattr(a, "shape") else len(a[0]) - 1
        with DavidsonEngine(n, lowest, max_dim_sub, gev=second is not None,
                            device=first.device.index if first.device.type != "cpu" else 0) as eng:
            eng.set_sparse(1, a, lower=lower, diagonals=diagonals)
            if second is not None:
                eng.set_sparse(2, second, lower=lower, diagonals=diagonals)
            return eng.solve(method, max_iterations, tolerance, initial_vectors=initial_vectors)
    if _is_device_csr(a) or _is_device_csr(second):
        # a matrix in device memory: an engine of its own, built on the GPU (DavidsonEngine.set_sparse)
        n = a.shape[0] if hasattr(a, "shape") else len(a[0]) - 1
        device = (a if _is_device_csr(a) else second).device.index
        with DavidsonEngine(n, lowest, max_dim_sub, gev=second is not None, device=device) as eng:
            eng.set_sparse(1, a, lower=lower, diagonals=diagonals)
            if second is not None:
                eng.set_sparse(2, second, lower=lower, diagonals=diagonals)
            return eng.solve(method, max_iterations, tolerance, initial_vectors=initial_vectors)
    n, rp, ci, vv = _sparse_input(a, None, lower)
    if second is not None:
        _, rpb, cib, vvb = _sparse_input(second, n, lower)
    else:
        rpb, cib, vvb = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1)
    evals = np.zeros(lowest)
    evecs = np.zeros((n, lowest), order="F")
    iters = C.c_int(-1)
    if initial_vectors is not None:
        x0 = _initial_vectors(initial_vectors, n, lowest)
        fortran_lib().fd_sparse_solve_guess(n, _i64(rp), _i32(ci), _dp(vv), int(second is not None), _i64(rpb), _i32(cib), _dp(vvb), 0,
                                            csr_flag_word(lower, diagonals), lowest, _method_code(method), max_iterations, tolerance,
                                            -1 if max_dim_sub is None else max_dim_sub, x0.shape[1], _dp(x0), _dp(evals), _dp(evecs),
                                            C.byref(iters))
        return evals, evecs, iters.value
    fortran_lib().fd_sparse_solve(n, _i64(rp), _i32(ci), _dp(vv), int(second is not None), _i64(rpb), _i32(cib), _dp(vvb), 0,
                                  csr_flag_word(lower, diagonals), lowest, _method_code(method), max_iterations, tolerance, -1 if max_dim_sub is None else max_dim_sub,
                                  _dp(evals), _dp(evecs), C.byref(iters))
    return evals, evecs, iters.value


def generalized_eigensolver_coo(rows, cols, vals, n, lowest, method, max_iterations, tolerance, max_dim_sub=None, second=None,
                                lower=False, initial_vectors=None, diagonals=False):
    """`call generalized_eigensolver(a_coo, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters [, max_dim_sub]
    [, b_coo])` (the coo_matrix specific of module davidson) with A as COO triples, 0-based, in any order, duplicates kept as separate
    terms: three arrays, or `rows` a scipy coo_matrix or a torch.sparse_coo_tensor and cols = vals = None (DavidsonEngine.set_coo
    says how each is read).  n: the order of the matrix; None when the first argument carries a shape.  `second`: B the same way - a
    tuple (rows, cols, vals) or one such object.  Triples in tensors on the GPU are built there.  lower, initial_vectors,
    diagonals: as for generalized_eigensolver_sparse.  Returns (eigenvalues, eigenvectors, iters)."""
    _check_method(method, a_sparse=True, blocks=(None, None), gev=second is not None, where="generalized_eigensolver_coo")
    a = rows if cols is None and vals is None else (rows, cols, vals)
    if n is None:
        if not hasattr(a, "shape"):
            raise ValueError("generalized_eigensolver_coo: n is needed when the triples come as three arrays")
        n = int(a.shape[0])
    on_gpu = [t for m in (a, second) if m is not None for t in (m if isinstance(m, tuple) else (m,))
              if type(t).__module__.startswith("torch") and t.device.type != "cpu"]
    with DavidsonEngine(n, lowest, max_dim_sub, gev=second is not None, device=on_gpu[0].device.index if on_gpu else 0) as eng:
        eng.set_coo(1, *(a if isinstance(a, tuple) else (a,)), lower=lower, diagonals=diagonals)
        if second is not None:
            eng.set_coo(2, *(second if isinstance(second, tuple) else (second,)), lower=lower, diagonals=diagonals)
        return eng.solve(method, max_iterations, tolerance, initial_vectors=initial_vectors)


def _hermitian_parts(a):
    """the three parts of a complex CSR operator given as a tuple (indptr, indices, data), an object with .indptr / .indices / .data (a
    scipy csr_matrix) or a torch.sparse_csr_tensor (on the CPU as numpy arrays, on a GPU as tensors), as they stand"""
    if is_torch_csr(a):
        return torch_csr_parts(a)
    if not isinstance(a, tuple):
        return a.indptr, a.indices, a.data
    return a


def hermitian_eigenpairs(theta, v, lowest, second=None, lower=False):
    """The `lowest` complex eigenpairs of H x = lambda S x from the 2 * lowest real Ritz pairs of its real form (Fortran:
    hermitian_eigenpairs): theta (2 * lowest,) ascending, v (2 n, 2 * lowest) real with real and imaginary parts interleaved,
    S-orthonormal in the real form.  second: S as a complex CSR matrix - a tuple (indptr, indices, data) or a scipy csr_matrix, 0-based,
    with lower=True only its entries with column <= row - or None for S = I.  Returns (eigenvalues (lowest,) ascending, eigenvectors
    complex (n, lowest) with X^H S X = I).
    The real form has every eigenvalue twice and the solver leaves an arbitrary rotation inside each pair, so Z = v[0::2] + i v[1::2]
    has the complex rank `lowest` only.  G = Z^H S Z equals I + iK with K real antisymmetric, its eigenvalues come in pairs 1 +- s, and
    the `lowest` largest are >= 1 even where the cut goes through a degenerate cluster: their vectors U and C = U diag(g^-1/2) give an
    S-orthonormal basis Z C of the space.  T = C^H (G diag(theta)) C, hermitised, = W Lambda W^H; X = Z C W.  O(n lowest^2) on the host."""
    theta = np.asarray(theta, dtype=np.float64)[:2 * lowest]
    v = np.asarray(v, dtype=np.float64)[:, :2 * lowest]
    if theta.size != 2 * lowest or v.ndim != 2 or v.shape[0] % 2 or v.shape[1] != 2 * lowest:
        raise ValueError(f"hermitian_eigenpairs: theta (2 * lowest,) and v (2 n, 2 * lowest) are needed, not {theta.shape} and {v.shape}")
    z = v[0::2] + 1j * v[1::2]
    if second is None:
        sz = z
    else:
        rp, ci, vv = check_hermitian(*_hermitian_parts(second), z.shape[0], 0, lower)
        rows = np.repeat(np.arange(z.shape[0]), np.diff(rp))
        sz = np.zeros_like(z)
        np.add.at(sz, rows, vv[:, None] * z[ci])
        if lower:
            off = ci != rows
            np.add.at(sz, ci[off], np.conj(vv[off])[:, None] * z[rows[off]])
    g = z.conj().T @ sz
    g = 0.5 * (g + g.conj().T)
    gw, u = np.linalg.eigh(g)
    c = u[:, lowest:] / np.sqrt(gw[lowest:])
    t = c.conj().T @ ((g * theta[None, :]) @ c)
    lam, w = np.linalg.eigh(0.5 * (t + t.conj().T))
    return lam, z @ (c @ w)


def _hermitian_guess(x, n, g_max):
    """initial_vectors= of a Hermitian solve: complex (n, g) -> real (2 n, 2 g): the g interleaved columns and their J-partners (the
    interleaved columns of i x) - one complex vector is two real ones"""
    x = np.asarray(x.cpu().numpy() if type(x).__module__.startswith("torch") else x)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    if x.dtype != np.complex128:
        raise TypeError(f"initial_vectors: x has dtype {x.dtype}, expected complex128")
    if x.ndim != 2 or x.shape[0] != n or x.shape[1] < 1:
        raise ValueError(f"initial_vectors: x must have shape ({n}, ncols), it has {x.shape}")
    x = x[:, :g_max]
    out = np.zeros((2 * n, 2 * x.shape[1]), order="F")
    out[0::2, :x.shape[1]], out[1::2, :x.shape[1]] = x.real, x.imag
    out[0::2, x.shape[1]:], out[1::2, x.shape[1]:] = -x.imag, x.real
    return out


def generalized_eigensolver_hermitian(indptr, indices, data, lowest, method, max_iterations, tolerance, max_dim_sub=None, second=None,
                                      lower=False, n=None, initial_vectors=None):
    """`call generalized_eigensolver(a_zcsr, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters [, max_dim_sub]
    [, b_zcsr])` (the zcsr_matrix specific of module davidson): the lowest eigenpairs of a complex Hermitian matrix A in CSR form,
    0-based - three arrays with data complex128, or `indptr` a scipy csr_matrix of complex dtype or a complex torch.sparse_csr_tensor
    and indices = data = None.  `second`: S of a generalized problem the same way.  A tensor on the GPU is built there.  The solve runs
    on the real form of order 2 n (DavidsonEngine.set_hermitian) for 2 * lowest real pairs, from which hermitian_eigenpairs takes the
    complex ones; max_dim_sub counts real columns (default 10 * 2 * lowest), iters is the real loop's count.  lower=True: only the
    entries with column <= row are given, for A and S.  initial_vectors: complex (n, g), staged as its g interleaved columns and their
    J-partners.  Returns (eigenvalues (lowest,), eigenvectors complex (n, lowest), iters)."""
    a = indptr if indices is None and data is None else (indptr, indices, data)
    if n is None:
        n = int(a.shape[0]) if hasattr(a, "shape") else len(a[0]) - 1
    on_gpu = [m for m in (a, second) if is_torch_csr(m) and m.device.type != "cpu"]
    with DavidsonEngine(2 * n, 2 * lowest, max_dim_sub, gev=second is not None, device=on_gpu[0].device.index if on_gpu else 0) as eng:
        eng.set_hermitian(1, a, lower=lower)
        if second is not None:
            eng.set_hermitian(2, second, lower=lower)
        guess = None if initial_vectors is None else _hermitian_guess(initial_vectors, n, lowest)
        theta, v, iters = eng.solve(method, max_iterations, tolerance, initial_vectors=guess)
    if second is not None and is_torch_csr(second) and second.device.type != "cpu":
        second = second.cpu()
    lam, x = hermitian_eigenpairs(theta, v, lowest, second, lower)
    return lam, x, iters


def _bsr_input(a, n, lower=False):
    """(b, indptr, indices, values) of a BSR operator given as a tuple (indptr, indices, data (nnzb, b, b) row-major blocks) or an object
    with .blocksize (a scipy bsr_matrix), 0-based, validated here (ValueError) - the Fortran door stops the process on an engine error.
    The values come back in Fortran order (values(m, k, p) = A_p[m, k]: each block transposed in memory) for the Fortran doors."""
    if is_torch_bsr(a):
        a = torch_bsr_parts(a)
    if hasattr(a, "blocksize"):
        a = (a.indptr, a.indices, a.data)
    indptr, indices, data = a
    if n is None:
        d = np.asarray(data)
        n = (len(indptr) - 1) * (d.shape[1] if d.ndim == 3 else 1)
    b, rp, ci, vv = check_bsr(indptr, indices, data, n, 0, lower)
    vf = np.ascontiguousarray(vv.transpose(0, 2, 1))
    return b, rp, ci, vf if vf.size else np.zeros(1)


def _is_device_bsr(a):
    return is_torch_bsr(a) and a.device.type != "cpu"


def generalized_eigensolver_bsr(indptr, indices, data, lowest, method, max_iterations, tolerance, max_dim_sub=None, second=None,
                                lower=False, n=None, initial_vectors=None):
    """`call generalized_eigensolver(a_bsr, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters [, max_dim_sub]
    [, b_bsr])` (the bsr_matrix specific of module davidson) with A in BSR form, 0-based: three arrays - data (nnzb, b, b), row-major
    blocks - or `indptr` an object with .indptr / .indices / .data / .blocksize (a scipy bsr_matrix) and indices = data = None.
    `second`: B the same way, with the same block size.  Either may also be a torch.sparse_bsr_tensor; one on the GPU is built there
    (DavidsonEngine.set_block_sparse on the tensor's device).  lower=True: only the blocks with block column <= block row are given,
    for A and B.  n: the order (default: block rows x b).  initial_vectors (n, g): the solve starts from these columns instead of unit
    vectors.  Returns (eigenvalues, eigenvectors, iters)."""
    _check_method(method, a_sparse=True, gev=second is not None, where="generalized_eigensolver_bsr")
    a = indptr if indices is None and data is None else (indptr, indices, data)
    if _is_device_bsr(a) or _is_device_bsr(second):
        # a matrix in device memory: an engine of its own, built on the GPU (DavidsonEngine.set_block_sparse)
        if n is None:
            if hasattr(a, "shape"):
                n = a.shape[0]
            else:
                n = (len(a[0]) - 1) * (np.asarray(a[2]).shape[1] if np.asarray(a[2]).ndim == 3 else 1)
        device = (a if _is_device_bsr(a) else second).device.index
        with DavidsonEngine(n, lowest, max_dim_sub, gev=second is not None, device=device) as eng:
            eng.set_block_sparse(1, a, lower=lower)
            if second is not None:
                eng.set_block_sparse(2, second, lower=lower)
            return eng.solve(method, max_iterations, tolerance, initial_vectors=initial_vectors)
    b, rp, ci, vv = _bsr_input(a, n, lower)
    n = (rp.size - 1) * b
    if second is not None:
        bb, rpb, cib, vvb = _bsr_input(second, n, lower)
        if bb != b:
            raise ValueError(f"BSR input: B has block size {bb}, A has {b}")
    else:
        rpb, cib, vvb = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1)
    evals = np.zeros(lowest)
    evecs = np.zeros((n, lowest), order="F")
    iters = C.c_int(-1)
    if initial_vectors is not None:
        x0 = _initial_vectors(initial_vectors, n, lowest)
        fortran_lib().fd_bsr_solve_guess(n, b, _i64(rp), _i32(ci), _dp(vv), int(second is not None), _i64(rpb), _i32(cib), _dp(vvb), 0,
                                         int(lower), lowest, _method_code(method), max_iterations, tolerance,
                                         -1 if max_dim_sub is None else max_dim_sub, x0.shape[1], _dp(x0), _dp(evals), _dp(evecs),
                                         C.byref(iters))
        return evals, evecs, iters.value
    fortran_lib().fd_bsr_solve(n, b, _i64(rp), _i32(ci), _dp(vv), int(second is not None), _i64(rpb), _i32(cib), _dp(vvb), 0, int(lower),
                               lowest, _method_code(method), max_iterations, tolerance, -1 if max_dim_sub is None else max_dim_sub,
                               _dp(evals), _dp(evecs), C.byref(iters))
    return evals, evecs, iters.value


def generalized_eigensolver_free(fun_matrix_gemv, n, lowest, method, max_iterations, tolerance, max_dim_sub,
                                 fun_second_matrix_gemv, initial_vectors=None):
    """Matrix-free specific with numpy callbacks X(n,k) -> Y(n,k) (reference: src/davidson.f90:277-337).  initial_vectors (n, g): the
    solve starts from these columns instead of unit vectors."""
    _check_method(method, gev=True, host_callbacks=True, where="generalized_eigensolver_free")
    lib = fortran_lib()

    def wrap(fn):
        def cb(nn, k, xp, yp):
            x = np.ctypeslib.as_array(xp, shape=(k, nn)).T
            y = np.ctypeslib.as_array(yp, shape=(k, nn))
            y[:, :] = np.asarray(fn(np.array(x, order="F"))).T
        return _CB(cb)

    fa, fb = wrap(fun_matrix_gemv), wrap(fun_second_matrix_gemv)
    evals = np.zeros(lowest)
    evecs = np.zeros((n, lowest), order="F")
    iters = C.c_int(-1)
    if initial_vectors is not None:
        x0 = _initial_vectors(initial_vectors, n, lowest)
        lib.fd_free_solve_guess(n, fa, fb, lowest, max_iterations, tolerance, 10 * lowest if max_dim_sub is None else max_dim_sub,
                                x0.shape[1], _dp(x0), _dp(evals), _dp(evecs), C.byref(iters))
        return evals, evecs, iters.value
    lib.fd_free_solve(n, fa, fb, lowest, max_iterations, tolerance, 10 * lowest if max_dim_sub is None else max_dim_sub, _dp(evals),
                      _dp(evecs), C.byref(iters))
    return evals, evecs, iters.value


class DavidsonEngine:
    """Device-resident problem (Fortran type `davidson_engine`): operators stay in HBM across solves.

    The third specific of the generic: `call generalized_eigensolver(engine, eigenvalues, eigenvectors,
    lowest, method, max_iterations, tolerance, iters, max_dim_sub)`.
    """

    def __init__(self, n, lowest, max_dim_sub=None, gev=False, device=0, rank=0, nranks=1, storage="full"):
        self.lib = fortran_lib()
        self.n, self.lowest = n, lowest
        self.max_dim = 10 * lowest if max_dim_sub is None else max_dim_sub
        self.gev = gev
        self.p = C.c_void_p(self.lib.fd_engine_create(n, lowest, self.max_dim, int(gev), device, rank, nranks))
        self.device = device
        self.nranks = nranks
        self.c = CEngine(handle=self.lib.fd_engine_handle(self.p), device=device)
        if storage != "full":
            self.lib.fd_engine_set_storage(self.p, {"full": 0, "symmetric": 1}[storage])

    def close(self):
        if self.p:
            self.lib.fd_engine_destroy(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def comm_init(self, unique_id: bytes):
        self.lib.fd_engine_comm_init(self.p, C.create_string_buffer(unique_id, 128))

    @staticmethod
    def _not_the_preconditioner(which, entry):
        """the entries that serve A and B only: refused here, because the Fortran doors stop the process on the engine's refusal"""
        if which == OP_M:
            raise ValueError(f"DavidsonEngine.{entry}: the preconditioner (which = 3, DAV_OP_M) is set with set_sparse, set_block_sparse, "
                             "set_device_operator or set_identity only")

    def set_dense(self, which, matrix):
        self._not_the_preconditioner(which, "set_dense")
        a = _f(matrix)
        assert a.shape == (self.n, self.n)
        self._note_blocks(which, None)
        self.lib.fd_engine_set_dense(self.p, which, _dp(a))

    def _note_blocks(self, which, b, sparse=False):
        """the block size of operator `which` while it is a BSR operator, None otherwise: what solve("BDPR") checks before the engine is
        called; sparse: it is a CSR or BSR operator, what solve("CHEB") checks"""
        self._blocks = getattr(self, "_blocks", [None, None, None])
        self._blocks[which - 1] = b
        self._sparse = getattr(self, "_sparse", [False, False, False])
        self._sparse[which - 1] = bool(sparse) or b is not None

    def _keep_map(self, which, keep_map):
        """the switch of the set call that follows (Fortran: engine_keep_value_map); what update_values knew of the operator goes"""
        self._note_blocks(which, None)
        self._kept = getattr(self, "_kept", {})
        self._kept.pop(which, None)
        self.lib.fd_engine_keep_value_map(self.p, which, int(keep_map))

    def set_sparse(self, which, indptr, indices=None, data=None, lower=False, keep_map=False, diagonals=False):
        """Operator A, B or the preconditioner M (which=1, 2, 3) as a symmetric matrix in CSR form, 0-based (Fortran: engine_set_sparse): three arrays,
        or `indptr` an object with .tocsr(), or a torch.sparse_csr_tensor - one on the engine's GPU is built there (Fortran:
        engine_set_sparse_device; a refused matrix raises DavidsonHipError and leaves the operator unset).  lower=True: only the
        entries with column <= row are given.  keep_map=True: the operator also keeps where its values came from (Fortran:
        engine_keep_value_map), so that update_values can replace them on the kept pattern.  diagonals=True: the matrix is stored by
        its diagonals (csr_matrix(..., diagonals=.true.)) - for stencils and banded matrices, also a scipy dia_matrix, for which the
        keyword stays explicit; a matrix with too many diagonals for its entries is refused (DavidsonHipError), never stored as CSR."""
        a = indptr if indices is None and data is None else (indptr, indices, data)
        if is_torch_coo(a):         # the triples as they stand: the COO path (set_coo)
            return self.set_coo(which, a, lower=lower, keep_map=keep_map, diagonals=diagonals)
        if _is_device_csr(a):
            return self._set_sparse_device(which, *torch_csr_parts(a), lower=lower, keep_map=keep_map, diagonals=diagonals)
        _, rp, ci, vv = _sparse_input(a, self.n, lower)
        self._keep_map(which, keep_map)
        self.lib.fd_engine_set_sparse(self.p, which, self.n, _i64(rp), _i32(ci), _dp(vv), 0, csr_flag_word(lower, diagonals))
        self._note_blocks(which, None, sparse=True)
        if keep_map:
            self._kept[which] = {"count": int(rp[-1] - rp[0]), "b": 1, "fortran_blocks": False}

    def _set_sparse_device(self, which, row_ptr, col_idx, vals, lower=False, keep_map=False, diagonals=False):
        rpb, cib, nnz = _device_csr_tensors(row_ptr, col_idx, vals, self.n, self.device)
        self._keep_map(which, keep_map)
        import torch
        torch.cuda.current_stream(row_ptr.device).synchronize()
        st = self.lib.fd_engine_set_sparse_device(self.p, which, self.n, row_ptr.data_ptr(), rpb, col_idx.data_ptr() or None, cib,
                                                  vals.data_ptr() or None, 0, csr_flag_word(lower, diagonals))
        if st != 0:
            raise DavidsonHipError(hip_lib().dav_last_error().decode())
        self._note_blocks(which, None, sparse=True)
        if keep_map:
            self._kept[which] = {"count": nnz, "b": 1, "fortran_blocks": False}

    def set_coo(self, which, rows, cols=None, vals=None, lower=False, keep_map=False, diagonals=False):
        """Operator A, B or the preconditioner M (which=1, 2, 3) as COO triples (rows[p], cols[p], vals[p]), 0-based, in any order and
        with duplicates, which stay separate terms in the order of p (Fortran: engine_set_sparse with a coo_matrix): three arrays, or a
        scipy coo_matrix (its .row, .col and .data as they stand - no sum_duplicates, no tocsr), or a torch.sparse_coo_tensor (its
        _indices() and _values() as they stand, coalesced or not).  Tensors on the engine's GPU are bucketed and sorted there (Fortran:
        engine_set_coo_device; a refused matrix raises DavidsonHipError and leaves the operator unset).  The operator equals, bit for
        bit, that of set_sparse on the CSR matrix a stable sort of the triples by row gives.  lower, diagonals: as for set_sparse.
        keep_map=True: update_values then takes the values in the order of the triples."""
        rows, cols, vals = coo_triples(rows, cols, vals)
        if type(vals).__module__.startswith("torch"):
            rb, cb, nnz = _device_coo_tensors(rows, cols, vals, self.device)
            self._keep_map(which, keep_map)
            import torch
            torch.cuda.current_stream(vals.device).synchronize()
            st = self.lib.fdx_engine_set_coo_device(self.p, which, self.n, nnz, rows.data_ptr() or None, rb, cols.data_ptr() or None, cb,
                                                   vals.data_ptr() or None, 0, csr_flag_word(lower, diagonals))
            if st != 0:
                raise DavidsonHipError(hip_lib().dav_last_error().decode())
        else:
            ri, ci, vv = check_coo(rows, cols, vals, self.n, 0, lower)
            nnz = int(vv.size)
            self._keep_map(which, keep_map)
            self.lib.fdx_engine_set_coo(self.p, which, self.n, nnz, _i32(ri), _i32(ci), _dp(vv) if nnz else (C.c_double * 1)(), 0,
                                       csr_flag_word(lower, diagonals))
        self._note_blocks(which, None, sparse=True)
        if keep_map:
            self._kept[which] = {"count": nnz, "b": 1, "fortran_blocks": False}

    def set_block_sparse(self, which, indptr, indices=None, data=None, lower=False, keep_map=False):
        """Operator A, B or the preconditioner M (which=1, 2, 3) as a symmetric matrix in BSR form, 0-based (Fortran: engine_set_sparse with a bsr_matrix):
        three arrays - data (nnzb, b, b), row-major blocks - or `indptr` an object with .blocksize (a scipy bsr_matrix), or a
        torch.sparse_bsr_tensor - one on the engine's GPU is built there (Fortran: engine_set_block_sparse_device; a refused matrix
        raises DavidsonHipError and leaves the operator unset).  lower=True: only the blocks with block column <= block row are given.
        keep_map=True: as for set_sparse; update_values then takes the blocks as this call does, (nnzb, b, b) row-major."""
        a = indptr if indices is None and data is None else (indptr, indices, data)
        if _is_device_bsr(a):
            return self._set_block_sparse_device(which, *torch_bsr_parts(a), lower=lower, keep_map=keep_map)
        b, rp, ci, vv = _bsr_input(a, self.n, lower)
        self._keep_map(which, keep_map)
        self.lib.fd_engine_set_block_sparse(self.p, which, self.n, b, _i64(rp), _i32(ci), _dp(vv), 0, int(lower))
        self._note_blocks(which, b)
        if keep_map:       # the Fortran door took the blocks in Fortran order: an update transposes them the same way
            self._kept[which] = {"count": int(rp[-1] - rp[0]) * b * b, "b": b, "fortran_blocks": True}

    def _set_block_sparse_device(self, which, row_ptr, col_idx, vals, lower=False, keep_map=False):
        b, rpb, cib, nnzb = _device_bsr_tensors(row_ptr, col_idx, vals, self.n, self.device)
        self._keep_map(which, keep_map)
        import torch
        torch.cuda.current_stream(row_ptr.device).synchronize()
        st = self.lib.fd_engine_set_block_sparse_device(self.p, which, self.n, b, row_ptr.data_ptr(), rpb, col_idx.data_ptr() or None, cib,
                                                        vals.data_ptr() or None, 0, int(lower), 1)
        if st != 0:
            raise DavidsonHipError(hip_lib().dav_last_error().decode())
        self._note_blocks(which, b)
        if keep_map:
            self._kept[which] = {"count": nnzb * b * b, "b": b, "fortran_blocks": False}

    def set_hermitian(self, which, a, lower=False, keep_map=False):
        """Operator A, B or the preconditioner M (which=1, 2, 3) of this engine of the real order 2 n as a complex Hermitian matrix of
        order n in CSR form, 0-based, through its real form (Fortran: engine_set_hermitian): a tuple (indptr, indices, data) with data
        complex128, a scipy csr_matrix of complex dtype or a complex torch.sparse_csr_tensor - one on the engine's GPU is built there
        (Fortran: engine_set_hermitian_device; a refused matrix raises DavidsonHipError and leaves the operator unset).  The operator
        is, bit for bit, the BSR operator of the blocks [[re, -im], [im, re]] with block size 2, and the methods see it as one.
        lower=True: only the entries with column <= row are given and the strict lower ones are mirrored as conjugates.
        keep_map=True: update_values then takes complex128 values in the order of this call."""
        if self.n % 2:
            raise ValueError(f"DavidsonEngine.set_hermitian: the engine's order {self.n} is odd; a Hermitian operator of order n needs an "
                             "engine of the real order 2 n")
        nc = self.n // 2
        parts = _hermitian_parts(a)
        if type(parts[2]).__module__.startswith("torch"):
            rpb, cib, nnz = _device_hermitian_tensors(*parts, nc, self.device)
            if keep_map:          # the positions of the diagonal entries, for the check update_values makes of host data
                import torch
                rows = torch.repeat_interleave(torch.arange(nc, device=parts[0].device), torch.diff(parts[0]).long())
                diag_pos = torch.nonzero(rows == parts[1][:nnz].long() - int(parts[0][0])).reshape(-1).cpu().numpy()
            self._keep_map(which, keep_map)
            import torch
            torch.cuda.current_stream(parts[0].device).synchronize()
            st = self.lib.fdh_engine_set_hermitian_device(self.p, which, nc, parts[0].data_ptr(), rpb, parts[1].data_ptr() or None, cib,
                                                          parts[2].data_ptr() or None, 0, int(lower))
            if st != 0:
                raise DavidsonHipError(hip_lib().dav_last_error().decode())
        else:
            rp, ci, vv = check_hermitian(*parts, nc, 0, lower)
            nnz = int(rp[-1] - rp[0])
            diag_pos = np.flatnonzero(ci[:nnz] == np.repeat(np.arange(nc), np.diff(rp)))
            self._keep_map(which, keep_map)
            self.lib.fdh_engine_set_hermitian(self.p, which, nc, _i64(rp), _i32(ci), vv.ctypes.data_as(C.c_void_p) if nnz else (C.c_double * 2)(),
                                              0, int(lower))
        self._note_blocks(which, 2, sparse=True)
        if keep_map:
            self._kept[which] = {"count": nnz, "b": 2, "fortran_blocks": False, "pairs": True, "diag_pos": diag_pos}

    def build_preconditioner(self, sigma=0.0, level=1):
        """The preconditioner M (slot 3) BUILT from the stored operators (Fortran: engine_build_preconditioner): the factorized sparse
        approximate inverse G^T G of A - sigma B on the pattern of tril(A)^level (the power of the lower triangle), level 1, 2 or 3 - at most 64 entries per row of G, a
        longer row is refused, never cut.  A was set by set_sparse / set_coo (CSR, not stored by diagonals), B the same way or not at
        all; A - sigma B must be positive definite (sigma at or below the lowest eigenvalue wanted).  solve("DPR") and solve("GJD")
        then apply it as they apply any M.  A snapshot of A, B and sigma: build again after update_values.  A refused build raises
        DavidsonHipError and leaves slot 3 unset.  Returns (entries of G, longest row of G, longest row of G^T)."""
        self._keep_map_forget(3)
        st = self.lib.fdp_engine_build_fsai(self.p, float(sigma), int(level))
        if st != 0:
            raise DavidsonHipError(hip_lib().dav_last_error().decode())
        nnz, row, col = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.lib.fdp_engine_fsai_info(self.p, C.byref(nnz), C.byref(row), C.byref(col))
        return nnz.value, row.value, col.value

    def build_block_preconditioner(self, sigma=0.0, level=1):
        """The preconditioner M (slot 3) BUILT from stored BLOCK operators (Fortran: engine_build_block_preconditioner): the block
        factorized sparse approximate inverse G^T G of A - sigma B on the pattern of tril(A)^level taken over the block index arrays,
        level 1, 2 or 3 - at most 64 scalar columns (64 // b blocks) per block row of G, a longer block row is refused, never cut.  A
        was set by set_block_sparse or set_hermitian (b = 2), B the same way with the same block size or not at all; A - sigma B must be
        positive definite.  solve("DPR") and solve("GJD") then apply it as they apply any M.  A snapshot of A, B and sigma: build again
        after update_values.  A refused build raises DavidsonHipError and leaves slot 3 unset.  Returns (block size, blocks of G,
        longest block row of G, longest block row of G^T)."""
        self._keep_map_forget(3)
        st = self.lib.fdq_engine_build_block_fsai(self.p, float(sigma), int(level))
        if st != 0:
            raise DavidsonHipError(hip_lib().dav_last_error().decode())
        b, nnzb, row, col = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.lib.fdq_engine_block_fsai_info(self.p, C.byref(b), C.byref(nnzb), C.byref(row), C.byref(col))
        return b.value, nnzb.value, row.value, col.value

    def _keep_map_forget(self, which):
        """what update_values and the method checks knew of operator `which` goes: it is no longer the sparse operator of a set call"""
        self._note_blocks(which, None)
        getattr(self, "_kept", {}).pop(which, None)

    def update_values(self, which, data):
        """New values of operator A (which=1), B (which=2) or M (which=3) on its kept pattern (Fortran: engine_update_sparse_values /
        engine_update_sparse_values_device): the operator was set by set_sparse / set_block_sparse with keep_map=True, and `data` is the
        data of that call with new numbers - for BSR (nnzb, b, b) row-major blocks, or the same flat.  A numpy array (or a CPU tensor)
        goes through the host entry, a torch tensor on the engine's GPU through the device entry; either works whichever way the
        operator was set.  float64 only - for an operator set by set_hermitian complex128 only, one value per entry, the diagonal entries
        real (host data: ValueError; device data: the engine's DavidsonHipError; both count entries and rows from 0) - (TypeError); a wrong length is a ValueError, an operator set without keep_map=True a
        DavidsonHipError - all before the engine is called, and the operator keeps its values.  Diagonal, applies and solves then equal
        bit for bit those of a fresh set call with `data`."""
        kept = getattr(self, "_kept", {}).get(which)
        if kept is None:
            raise DavidsonHipError(f"update_values: operator {which} was not set with keep_map=True (dav_keep_value_map): it keeps no "
                                   "value map")
        pairs = kept.get("pairs", False)
        host, dev = update_values_array(data, kept["count"], self.device, "update_values", pairs=pairs)
        b = kept["b"]
        if dev is not None:
            import torch
            if kept["fortran_blocks"] and b > 1:
                dev = dev.reshape(-1, b, b).transpose(1, 2).contiguous()
            torch.cuda.current_stream(dev.device).synchronize()
            st = self.lib.fd_engine_update_values_device(self.p, which, dev.data_ptr() or None)
            if st != 0:
                raise DavidsonHipError(hip_lib().dav_last_error().decode())
            return
        if kept["fortran_blocks"] and b > 1:
            host = np.ascontiguousarray(host.reshape(-1, b, b).transpose(0, 2, 1)).reshape(-1)
        if pairs:          # complex128 values: the (re, im) pairs as they lie, 2 doubles each
            # the engine's one refusal of values, made here: the Fortran door of host data stops the process on it
            bad = kept["diag_pos"][~(host[kept["diag_pos"]].imag == 0.0)]
            if bad.size:
                raise ValueError(f"update_values: diagonal entry {int(bad[0])} has the imaginary part {float(host[bad[0]].imag)!r}: the "
                                 "diagonal of a Hermitian matrix is real")
            self.lib.fd_engine_update_values(self.p, which, host.ctypes.data_as(C.c_void_p) if host.size else (C.c_double * 2)(), 2 * host.size)
            return
        self.lib.fd_engine_update_values(self.p, which, _dp(host) if host.size else (C.c_double * 1)(), host.size)

    def set_correction_policy(self, policy):
        """"all" = the reference's policy (default); "unconverged" = opt-in: correct only the wanted pairs
        that have not converged; "locking" = opt-in (standard problems): converged wanted pairs are locked and the
        search space is kept orthogonal to them (Fortran: engine_set_correction_policy)."""
        self.lib.fd_engine_set_policy(self.p, {"all": 0, "unconverged": 1, "locking": 2}[policy])

    def set_inner_precision(self, bits):
        """32: the sweeps inside the GJD correction read an fp32 copy of the stored symmetric tiles (Fortran:
        engine_set_inner_precision); 64 (default): the reference's precision throughout."""
        self.lib.fd_engine_set_inner_precision(self.p, bits)

    def set_device_rr(self, on=True):
        """Rayleigh-Ritz on the device (Fortran: engine_set_device_rr); default off = host LAPACK as the reference."""
        self.lib.fd_engine_set_device_rr(self.p, int(on))

    def read_matrix(self, which, path, fmt="text"):
        """Operator from a file, streamed to HBM (Fortran: engine_read_matrix): "text" = the reference's
        write_matrix/read_matrix dump format, "f64" = raw row-major float64."""
        self._not_the_preconditioner(which, "read_matrix")
        self._note_blocks(which, None)
        self.c.set_dense_file(which - 1, path, fmt)

    def _set_op(self, which, kind, seed, sparsity, diag_val):
        self._note_blocks(which, None)
        self.lib.fd_engine_set_operator(self.p, which, kind, seed, sparsity, *_optional(diag_val))

    def generate_diagonal_dominant(self, which, sparsity, diag_val=None, seed=1):
        """generate_diagonal_dominant(n, sparsity[, diag_val]) built directly in HBM."""
        self._not_the_preconditioner(which, "generate_diagonal_dominant")
        self._set_op(which, 0, seed, sparsity, diag_val)

    def set_hashed_operator(self, which, sparsity, diag_val=None, seed=1):
        self._not_the_preconditioner(which, "set_hashed_operator")
        self._set_op(which, 1, seed, sparsity, diag_val)

    def set_harness_operator(self, which):
        self._not_the_preconditioner(which, "set_harness_operator")
        self._set_op(which, 2, 0, 0.0, None)

    def set_identity(self, which):
        """B = I (which = 2), or the preconditioner M = I (which = 3: "DPR" then corrects with T = R)."""
        self._set_op(which, 3, 0, 0.0, None)

    def set_device_operator(self, which, fn, ctx, diag=None):
        """The caller's own operator as a block apply on device memory (engine_set_device_operator; which = 1 / 2 / 3).  diag: the
        operator's diagonal; the preconditioner's (which = 3) is not read and may be None."""
        self._note_blocks(which, None)
        self.c.set_operator_device(which - 1, fn, ctx, diag)

    def set_initial_vectors(self, x):
        """The next solve starts from the columns of x (n rows) instead of unit vectors (Fortran: engine_set_initial_vectors /
        engine_set_initial_vectors_device): a numpy array goes through the host entry, a torch tensor on the engine's GPU through the
        device entry.  One-shot.  float64 only (TypeError); a wrong row count is a ValueError before any engine call; the engine's
        refusal - an entry that is not finite, a column that is entirely zero - a DavidsonHipError, and a guess staged earlier stays
        staged.  Of a guess wider than the start basis (2 * lowest columns) the leading columns are used."""
        host, dev = guess_array(x, self.n, self.device, "initial_vectors")
        width = 2 * self.lowest                 # (the engine's basis always holds the start basis)
        if dev is not None:
            import torch
            t, ld, ncols = dev
            torch.cuda.current_stream(t.device).synchronize()
            st = self.lib.fd_engine_set_initial_vectors_device(self.p, t.data_ptr() or None, ld, min(ncols, width))
        else:
            host = np.asfortranarray(host[:, :width])
            st = self.lib.fd_engine_set_initial_vectors(self.p, _dp(host), host.shape[1])
        if st != 0:
            raise DavidsonHipError(hip_lib().dav_last_error().decode())

    def keep_result_as_guess(self, on=True):
        """Sticky (Fortran: engine_keep_result_as_guess): while on, every solve starts from the Ritz vectors the previous solve on this
        engine left in HBM - nothing is copied; update_values and the set calls keep them."""
        self.lib.fd_engine_keep_result_as_guess(self.p, int(on))

    def solve(self, method="DPR", max_iterations=1000, tolerance=1e-8, want_vectors=True, initial_vectors=None, reuse_vectors=None):
        """initial_vectors: see set_initial_vectors (a one-shot guess for this solve).  reuse_vectors: True / False turns
        keep_result_as_guess on / off before the solve (sticky), None leaves it as it is; with it on and no initial_vectors the solve
        starts from the previous solve's Ritz vectors when they are still in place.  method "BDPR": the block-diagonal form of DPR,
        for operators set with set_block_sparse (ValueError otherwise, before the engine is called).  method "CHEB" / "CHEB<d>": the
        Chebyshev-filtered correction of degree d (1..64, default 10) for a standard problem whose A was set with set_sparse or
        set_block_sparse (ValueError otherwise, before the engine is called).  method "LCHEB" / "LCHEB<d>": the same correction with
        a Lanczos bound, for a standard problem whose A is anything the engine applies on the device - set_dense, set_device_operator,
        set_hashed_operator, set_sparse, set_block_sparse ... (a generalized problem: ValueError before the engine is called)."""
        if _parse_method(method)[0] > 2:         # DPR, GJD and names that are none ask nothing of what the engine holds
            # (BDPR's checks read A and B only: the preconditioner's blocks are no concern of a method that does not apply it)
            _check_method(method, a_sparse=getattr(self, "_sparse", [False, False, False])[0],
                          blocks=getattr(self, "_blocks", [None, None, None])[:2], gev=self.gev, n=self.n, nranks=self.nranks, where="DavidsonEngine.solve")
        if reuse_vectors is not None:
            self.keep_result_as_guess(bool(reuse_vectors))
        if initial_vectors is not None:
            self.set_initial_vectors(initial_vectors)
        evals = np.zeros(self.lowest)
        evecs = np.zeros((self.n, self.lowest) if want_vectors else (1, 1), order="F")
        iters = C.c_int(-1)
        self.lib.fd_engine_solve(self.p, self.lowest, _method_code(method), max_iterations, tolerance, self.max_dim, _dp(evals),
                                 int(want_vectors), _dp(evecs), C.byref(iters))
        return evals, (evecs if want_vectors else None), iters.value


# ---- helper modules (array_utils / lapack_wrapper) --------------------------------------------------
def generate_diagonal_dominant(m, sparsity, diag_val=None, seed=1):
    out = np.zeros((m, m), order="F")
    fortran_lib().fd_generate_diagonal_dominant(m, sparsity, *_optional(diag_val), seed, _dp(out))
    return out


def lapack_generalized_eigensolver(mtx, stx=None):
    mtx = _f(mtx)
    n = mtx.shape[0]
    s = _f(stx) if stx is not None else np.zeros((1, 1), order="F")
    w = np.zeros(n)
    v = np.zeros((n, n), order="F")
    fortran_lib().fd_lapack_eigensolver(n, _dp(mtx), int(stx is not None), _dp(s), _dp(w), _dp(v))
    return w, v


def lapack_rayleigh_ritz(mtx, nvec, stx=None):
    """The Rayleigh-Ritz solver of the outer loop: lowest `nvec` pairs (first nvec entries / columns valid)."""
    mtx = _f(mtx)
    n = mtx.shape[0]
    s = _f(stx) if stx is not None else np.zeros((1, 1), order="F")
    w = np.zeros(n)
    v = np.zeros((n, n), order="F")
    fortran_lib().fd_lapack_rayleigh_ritz(n, _dp(mtx), int(stx is not None), _dp(s), nvec, _dp(w), _dp(v))
    return w[:nvec], v[:, :nvec]


def lapack_qr(basis):
    q = _f(basis).copy(order="F")
    fortran_lib().fd_lapack_qr(q.shape[0], q.shape[1], _dp(q))
    return q


def lapack_solver(arr, brr):
    a = _f(arr).copy(order="F")
    b = np.array(brr, dtype=np.float64).reshape(-1, 1).copy(order="F")
    fortran_lib().fd_lapack_solver(a.shape[0], _dp(a), _dp(b))
    return b[:, 0]


def lapack_matmul(transA, transB, arr, brr):
    a, b = _f(arr), _f(brr)
    m = a.shape[1] if transA == "T" else a.shape[0]
    k = a.shape[0] if transA == "T" else a.shape[1]
    n = b.shape[0] if transB == "T" else b.shape[1]
    c = np.zeros((m, n), order="F")
    fortran_lib().fd_lapack_matmul(int(transA == "T"), int(transB == "T"), m, k, n, _dp(a), _dp(b), _dp(c))
    return c


def lapack_sort(id_, vector):
    v = np.array(vector, dtype=np.float64)
    keys = np.zeros(v.size, dtype=np.int32)
    fortran_lib().fd_lapack_sort(v.size, int(id_ == "D"), _dp(v), keys.ctypes.data_as(C.POINTER(C.c_int)))
    return keys, v


def generate_preconditioner(diag, dim_sub):
    d = np.array(diag, dtype=np.float64)
    out = np.zeros((d.size, dim_sub), order="F")
    fortran_lib().fd_generate_preconditioner(d.size, _dp(d), dim_sub, _dp(out))
    return out


def norm(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    res = C.c_double()
    fortran_lib().fd_norm(v.size, _dp(v), C.byref(res))
    return res.value
