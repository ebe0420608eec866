"""GPU: every block-product kernel variant against an exact or rigorously bounded reference, inside write fences.

The answers below do not depend on the order of summation, so they hold for every schedule, knob setting and rank count:
  1. stored operators (full storage, symmetric tiles, from device memory, the fp32 tile copy of the inner sweeps) on integer data
     (tests/exact_inputs.py): bitwise the integer product;
  2. generated operators (hashed, dav_set_dense_generated, a partly resident B) on blocks with at most two nonzeros +-2^p per column
     at tile- and slab-edge rows: every output entry is one rounding of two exact products - bitwise the oracle's entries times X;
  3. every variant again on graded float data (D A D, D = 2^+-20 per row) within the componentwise bound gamma_n (|A| |X|) of a
     long-double reference (the fp32 tiles: plus the rounding of A to fp32; the harness operator: plus its entries' allowance);
  4. write fences on every apply (source panel bitwise unchanged, destination columns outside [d0, d0 + k) untouched, padding rows of
     the result zero through the engine's own Gram product), and on gram / panel_transform;
  5. CSR and BSR with NaN in chosen rows of X: NaN exactly in the output rows whose stored pattern reads one, every other row exact;
  6. the exact cases on 2, 3 and 5 ranks (threads of one process, loopback collectives).
The DAV_* knobs are read at dav_create, so each case sets them with monkeypatch before its engine exists.  DISPATCH maps every kernel
instantiation of these products to the cases meant to reach it; profiles/exact_products_kernel_coverage.csv is a rocprofv3 kernel
trace of one run of this module, and tests/test_exact_products_coverage.py checks the two against each other."""
import zlib
from typing import NamedTuple

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.distributed import RowPartition
from fortran_davidson_amd.engine_c import OP_A, OP_B, PANEL_V, PANEL_W
from exact_inputs import (SENTINEL, exact_dense_product, exact_sparse_product, fenced_apply, gamma, gram_is_exact, int_block, mismatch,
                          run_ranks, same_bits, sym_int_matrix, touched_rows, unit_block)
from oracle import davidson_oracle as O

pytestmark = pytest.mark.gpu

R2, R4 = {"DAV_SYM_R": "2"}, {"DAV_SYM_R": "4"}


def _b(v):
    return "true" if v else "false"


# kernel instantiations by their demangled names (what a kernel trace lists, up to the argument list)
def mvd(g):
    return f"matvec_dense_kernel<{g}>"


def free(g, kind):                      # kind: 2 hashed, 3 harness (common.h: DAV_KIND_*)
    return f"matvec_free_kernel<{g}, {kind}>"


def s8(gen):
    return f"matvec_sym8_kernel<{_b(gen)}>"


def s9(r, gen=False, f32=False, m4=False, harn=0):
    return f"matvec_sym9_kernel<{r}, {_b(gen)}, {_b(f32)}, {_b(m4)}, {harn}>"


def sw(nb, tall=False, f32=False, gen=0):
    return f"matvec_symw_kernel<{nb}, {_b(tall)}, {_b(f32)}, {gen}>"


SLAB, SYMRED, SYM9RED = "slab_reduce_kernel", "sym_reduce_kernel", "sym9_reduce_kernel"


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _set_env(monkeypatch, env):
    for key, val in env.items():
        monkeypatch.setenv(key, val)


def _apply_fn(e, inner=False, which=OP_A):
    f = e.apply_inner if inner else e.apply
    return lambda sp, c0, k, dp, d0: f(which, sp, c0, k, dp, d0)


# ---- 1. stored operators, exact integers ---------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    storage: int            # 0: full, 1: symmetric tiles
    env: dict
    n: int
    k: int
    c0: int
    d0: int
    reaches: tuple          # kernel instantiations this case is meant to launch
    src: str = "host"       # "host" | "dev" (dav_set_dense_dev from a torch tensor)
    inner: bool = False     # dav_apply_inner at inner precision 32: the fp32 tile copy up to 16 columns

    @property
    def cols(self):         # panel columns: room for the NaN / sentinel columns on both sides and a wider stale apply
        return max(self.c0, self.d0) + self.k + 17


# Orders: 1, 15 / 16 / 17 (slabs padded to 16), 255 / 256 / 257 / 511 / 513 (SYM_TB = 256), 769, 1025, 1300 and 2305 - 1, 2, 3, 4, 5, 6
# and 10 block rows: the last super row of two block rows ragged (1, 3, 5), of four ragged by 1 (1025), 2 (257, 1300, 2305) or 3 (513).
# Widths: 1 / 2 / 4 column groups, each full and partly filled (24, 31 = 16 + 15, 63), the 3 -> 4 promotion, the splits at 32 and 64.
STORED = [
    # full storage: row slabs, matvec_dense_kernel<column groups> and the fixed-order sum of the split slabs
    Case("full-n1-k1", 0, {}, 1, 1, 0, 0, (mvd(1), SLAB)),
    Case("full-n1-k17", 0, {}, 1, 17, 3, 1, (mvd(2),)),
    Case("full-n15-k1", 0, {}, 15, 1, 0, 0, (mvd(1), SLAB)),
    Case("full-n16-k9", 0, {}, 16, 9, 3, 1, (mvd(1),)),
    Case("full-n17-k17", 0, {}, 17, 17, 1, 5, (mvd(2),)),
    Case("full-n255-k33", 0, {}, 255, 33, 5, 3, (mvd(4),)),
    Case("full-n257-k65", 0, {}, 257, 65, 1, 7, (mvd(4), mvd(1))),
    Case("full-n513-k96", 0, {}, 513, 96, 3, 1, (mvd(4), mvd(2))),
    Case("full-n2305-k31", 0, {}, 2305, 31, 7, 9, (mvd(2),)),
    Case("full-dev-n511-k40", 0, {}, 511, 40, 1, 3, (mvd(4),), src="dev"),
    # symmetric tiles, one block row per workgroup (the default below 64 block rows); 32 columns per launch as paired groups
    Case("sym-n1-k4", 1, {}, 1, 4, 1, 1, (s8(False), SYMRED)),
    Case("sym-n16-k4", 1, {}, 16, 4, 1, 1, (s8(False), SYMRED)),
    Case("sym-n1300-k32", 1, {}, 1300, 32, 1, 3, (s8(False),)),
    Case("sym-n769-k63", 1, {}, 769, 63, 3, 1, (s8(False),)),
    Case("sym-n256-k8", 1, {}, 256, 8, 0, 3, (s8(False),)),
    Case("sym-n257-k65", 1, {}, 257, 65, 3, 1, (s8(False),)),
    Case("sym-n1300-k48", 1, {}, 1300, 48, 5, 3, (s8(False),)),
    Case("sym-n2305-k17", 1, {}, 2305, 17, 1, 1, (s8(False),)),
    Case("sym-nopair-n511-k33", 1, {"DAV_SYM_PAIR": "0"}, 511, 33, 1, 5, (s8(False),)),
    Case("sym-dev-n513-k15", 1, {}, 513, 15, 3, 3, (s8(False),), src="dev"),
    # two block rows per workgroup: the one-wave-per-SIMD kernel (16 columns per workgroup; 32 as two groups; 64 as four in one launch)
    Case("r2-n257-k16", 1, R2, 257, 16, 1, 3, (sw(1), SYM9RED)),
    Case("r2-n513-k4", 1, R2, 513, 4, 3, 1, (sw(1),)),
    Case("r2-n1300-k9", 1, R2, 1300, 9, 5, 7, (sw(1),)),
    Case("r2-n513-k33", 1, R2, 513, 33, 1, 1, (sw(2), sw(1))),
    Case("r2-n1-k24", 1, R2, 1, 24, 1, 1, (sw(2),)),                     # second group partly filled (24 = 16 + 8)
    Case("r2-n513-k24", 1, R2, 513, 24, 5, 3, (sw(2),)),
    Case("r2-n1025-k32", 1, R2, 1025, 32, 3, 1, (sw(2),)),
    Case("r2-n1300-k63", 1, R2, 1300, 63, 1, 5, (sw(2),)),               # 32 + 31 columns
    Case("r2-n2305-k64", 1, R2, 2305, 64, 1, 3, (sw(2),)),
    Case("r2-n513-k96", 1, R2, 513, 96, 3, 5, (sw(2),)),
    Case("r2-noquad-n1300-k65", 1, {**R2, "DAV_SYM_QUAD": "0"}, 1300, 65, 1, 1, (sw(2), sw(1))),
    Case("r2-wide0-n2305-k40", 1, {**R2, "DAV_SYM_WIDE": "0"}, 2305, 40, 3, 1, (s9(2),)),
    Case("r2-wide0-n513-k8", 1, {**R2, "DAV_SYM_WIDE": "0"}, 513, 8, 1, 1, (s9(2),)),
    Case("r2-wide1-n1300-k15", 1, {**R2, "DAV_SYM_WIDE": "1"}, 1300, 15, 1, 3, (s9(2),)),
    # four block rows per workgroup: the 4x4x4 MFMA at <= 8 columns (DAV_SYM_MFMA4=0: the 16-wide one), the tall wide kernel at 9-16
    Case("r4-n2305-k8", 1, R4, 2305, 8, 1, 1, (s9(4, m4=True),)),
    Case("r4-n257-k1", 1, R4, 257, 1, 0, 0, (s9(4, m4=True),)),
    Case("r4-mfma16-n1300-k7", 1, {**R4, "DAV_SYM_MFMA4": "0"}, 1300, 7, 3, 5, (s9(4),)),
    Case("r4-n1300-k16", 1, R4, 1300, 16, 1, 3, (sw(1, tall=True),)),
    Case("r4-n2305-k9", 1, R4, 2305, 9, 5, 1, (sw(1, tall=True),)),
    Case("r4-n1-k8", 1, R4, 1, 8, 1, 3, (s9(4, m4=True),)),
    Case("r4-n513-k8", 1, R4, 513, 8, 3, 1, (s9(4, m4=True),)),
    Case("r4-mfma16-n1025-k5", 1, {**R4, "DAV_SYM_MFMA4": "0"}, 1025, 5, 1, 1, (s9(4),)),
    Case("r4-n1025-k16", 1, R4, 1025, 16, 1, 3, (sw(1, tall=True),)),
    Case("r4-n513-k12", 1, R4, 513, 12, 3, 5, (sw(1, tall=True),)),
    # the fp32 copy of the tiles (inner sweeps of up to 16 columns): entries widened to fp64 - exact on this data as well
    Case("f32-n1300-k16", 1, {}, 1300, 16, 1, 1, (sw(1, f32=True), "tiles_to_f32_kernel"), inner=True),
    Case("f32-n513-k9", 1, R2, 513, 9, 3, 1, (sw(1, f32=True),), inner=True),
    Case("f32-wide32off-n513-k9", 1, {"DAV_SYM_WIDE32": "0"}, 513, 9, 1, 3, (s9(2, f32=True),), inner=True),
    Case("f32-r4-n2305-k8", 1, R4, 2305, 8, 1, 1, (s9(4, f32=True, m4=True),), inner=True),
    Case("f32-n1300-k33", 1, {}, 1300, 33, 3, 1, (s8(False), sw(1, f32=True)), inner=True),     # 32 columns on the fp64 tiles, then 1
    Case("f32-n1300-k32", 1, {}, 1300, 32, 1, 1, (s8(False),), inner=True),
    Case("f32-r4-n1025-k3", 1, R4, 1025, 3, 1, 3, (s9(4, f32=True, m4=True),), inner=True),
]
STORED_BY_NAME = {c.name: c for c in STORED}
_MATRICES = {}


def _stored_inputs(case):
    if case.n not in _MATRICES:
        _MATRICES[case.n] = sym_int_matrix(case.n, np.random.default_rng(_seed("A", case.n)))
    rng = np.random.default_rng(_seed("X", case.name))
    return _MATRICES[case.n], int_block(case.n, case.k, rng), unit_block(case.n, case.k, rng)


def _set_stored(e, case, a):
    e.set_storage(case.storage)
    if case.src == "dev":
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()          # row-major A^T = column-major A
        e.set_dense_dev(OP_A, t.data_ptr(), case.n)
        del t
    else:
        e.set_dense_host(OP_A, a)
    if case.inner:
        e.set_inner_precision(32)


def _stored_run(e, case, a, x, xs):
    """(W, fence messages, W of the unit block, gram of that W) - the same calls on every rank"""
    _set_stored(e, case, a)
    ap = _apply_fn(e, case.inner)
    w, msgs = fenced_apply(e, x, case.c0, case.d0, case.cols, ap, stale=case.k + 16)
    ws, msgs2 = fenced_apply(e, xs, case.c0, case.d0, case.cols, ap)
    return w, msgs + msgs2, ws, e.gram(PANEL_W, case.d0, case.k, PANEL_W, case.d0, case.k)


def _check_stored(case, out, ref, refs):
    w, msgs, ws, g = out
    assert not msgs, (case.name, msgs)
    assert np.array_equal(w, ref), (case.name, mismatch(w, ref))
    assert np.array_equal(ws, refs), (case.name, mismatch(ws, refs))
    assert gram_is_exact(g, ws), (case.name, "gram(W, W) != W^T W: padding rows of the result are not zero")


@pytest.mark.parametrize("name", [c.name for c in STORED])
def test_stored_operator_products_are_exact(name, monkeypatch):
    case = STORED_BY_NAME[name]
    _set_env(monkeypatch, case.env)
    a, x, xs = _stored_inputs(case)
    with fd.CEngine(n=case.n, max_cols=case.cols) as e:
        out = _stored_run(e, case, a, x, xs)
    _check_stored(case, out, exact_dense_product(a, x), exact_dense_product(a, xs))


# the dealt-out symmetric tiles with their reduce-scatter (every schedule) and the row slabs of full storage
RANK_CASES = ["full-n513-k96", "sym-n1300-k48", "r2-n2305-k64", "r2-n513-k33", "r2-n513-k24", "r2-n1300-k63", "r2-wide0-n2305-k40",
              "r4-n2305-k8", "r4-n1300-k16", "r4-n1025-k16"]


@pytest.mark.parametrize("nranks", [2, 3, 5])
@pytest.mark.parametrize("name", RANK_CASES)
def test_stored_operator_products_are_exact_over_ranks(name, nranks, monkeypatch):
    case = STORED_BY_NAME[name]
    _set_env(monkeypatch, case.env)
    a, x, xs = _stored_inputs(case)
    outs = run_ranks(nranks, lambda r: fd.CEngine(n=case.n, max_cols=case.cols, rank=r, nranks=nranks),
                     lambda r, e: _stored_run(e, case, a, x, xs))
    ref, refs = exact_dense_product(a, x), exact_dense_product(a, xs)
    for out in outs:
        _check_stored(case, out, ref, refs)


# ---- 2. generated operators, two exact terms per output entry -----------------------------------------------------------------------
SEED, SPARSITY = 13, 1e-2


class GenCase(NamedTuple):
    name: str
    storage: int
    kind: str               # "hashed" | "generated" (dav_set_dense_generated: stored tiles made on the device) | "resident" (B)
    env: dict
    n: int
    k: int
    c0: int
    d0: int
    reaches: tuple

    @property
    def cols(self):
        return max(self.c0, self.d0) + self.k + 17


GEN = [
    GenCase("free-hashed-n1300-k9", 0, "hashed", {}, 1300, 9, 1, 3, (free(1, 2), SLAB)),
    GenCase("free-hashed-n513-k17", 0, "hashed", {}, 513, 17, 3, 1, (free(2, 2),)),
    GenCase("free-hashed-n2305-k40", 0, "hashed", {}, 2305, 40, 1, 1, (free(4, 2),)),
    GenCase("generated-full-n2305-k8", 0, "generated", {}, 2305, 8, 3, 5, (mvd(1),)),
    GenCase("generated-sym-n1300-k24", 1, "generated", {}, 1300, 24, 1, 3, ("generate_sym_tiles_kernel", s8(False))),
    GenCase("sym-hashed-n1300-k8", 1, "hashed", {}, 1300, 8, 1, 1, (s8(True),)),
    GenCase("sym-hashed-r2-n2305-k16", 1, "hashed", R2, 2305, 16, 3, 1, (s9(2, gen=True),)),
    GenCase("sym-hashed-r2-n2305-k40", 1, "hashed", R2, 2305, 40, 1, 5, (sw(2, gen=1),)),
    GenCase("sym-hashed-r2-n1300-k24", 1, "hashed", R2, 1300, 24, 3, 1, (sw(2, gen=1),)),
    GenCase("sym-hashed-r2-n1025-k63", 1, "hashed", R2, 1025, 63, 1, 3, (sw(2, gen=1),)),
    GenCase("sym-hashed-r2-genwide0-n1300-k33", 1, "hashed", {**R2, "DAV_SYM_GEN_WIDE": "0"}, 1300, 33, 1, 1, (s9(2, gen=True),)),
    GenCase("sym-hashed-r4-n2305-k8", 1, "hashed", R4, 2305, 8, 1, 3, (s9(4, gen=True, m4=True),)),
    # B = the unit-diagonal generator with the tiles of its longest block rows resident: stored part, then the generated part added
    GenCase("resident-b-n2600-k24", 1, "resident", {"DAV_B_RESIDENT": "85"}, 2600, 24, 3, 1, (s8(False), s8(True))),
]
GEN_BY_NAME = {c.name: c for c in GEN}


def edge_rows(n):
    """0, 255, 256, 257, n - 1 and the first and last row of every rank's slab for 2, 3 and 5 ranks"""
    rows = {0, 255, 256, 257, n - 1}
    for p in (2, 3, 5):
        for r in range(p):
            part = RowPartition(n, p, r)
            if part.nloc > 0:
                rows |= {part.row0, part.row0 + part.nloc - 1}
    return np.array(sorted(r for r in rows if r < n))


def two_term_block(n, k):
    """at most two nonzeros +-2^p per column, at edge rows: A X is one rounding of two exact products, in any order of summation"""
    rows = edge_rows(n)
    m = rows.size
    x = np.zeros((n, k), order="F")
    for c in range(k):
        r1, r2 = rows[c % m], rows[(3 * c + 1) % m]
        x[r1, c] = (-1.0) ** c * 2.0 ** (c % 7 - 3)
        if r2 != r1:
            x[r2, c] = (-1.0) ** (c // 2) * 2.0 ** ((c // 7) % 5 - 2)
    return x, rows


def _gen_reference(case, x, rows):
    ar = O.generate_diagonal_dominant(case.n, SPARSITY, 1.0 if case.kind == "resident" else None, seed=SEED, rows=rows)
    return np.asfortranarray(ar.T @ x[rows])         # rows of the symmetric matrix = its columns; zeros add exactly


def _set_generated(e, case):
    e.set_storage(case.storage)
    if case.kind == "hashed":
        e.set_operator_hashed(OP_A, SEED, SPARSITY)
    elif case.kind == "generated":
        e.set_dense_generated(OP_A, SEED, SPARSITY)
    else:
        e.set_operator_hashed(OP_B, SEED, SPARSITY, 1.0)
    return OP_B if case.kind == "resident" else OP_A


def _gen_run(e, case, x):
    which = _set_generated(e, case)
    w, msgs = fenced_apply(e, x, case.c0, case.d0, case.cols, _apply_fn(e, which=which), stale=case.k + 16)
    return w, msgs, e.resident_fraction(which) if case.kind == "resident" else None


@pytest.mark.parametrize("name", [c.name for c in GEN])
def test_generated_operator_products_are_exact(name, monkeypatch):
    case = GEN_BY_NAME[name]
    _set_env(monkeypatch, case.env)
    x, rows = two_term_block(case.n, case.k)
    with fd.CEngine(n=case.n, max_cols=case.cols, gev=case.kind == "resident") as e:
        w, msgs, frac = _gen_run(e, case, x)
    assert not msgs, msgs
    ref = _gen_reference(case, x, rows)
    assert np.array_equal(w, ref), mismatch(w, ref)
    if case.kind == "resident":
        assert 0.0 < frac < 1.0, frac                   # both parts ran


GEN_RANK_CASES = ["free-hashed-n2305-k40", "sym-hashed-n1300-k8", "sym-hashed-r2-n2305-k40", "sym-hashed-r2-n1300-k24", "sym-hashed-r4-n2305-k8",
                  "resident-b-n2600-k24"]


@pytest.mark.parametrize("nranks", [2, 3, 5])
@pytest.mark.parametrize("name", GEN_RANK_CASES)
def test_generated_operator_products_are_exact_over_ranks(name, nranks, monkeypatch):
    case = GEN_BY_NAME[name]
    _set_env(monkeypatch, case.env)
    x, rows = two_term_block(case.n, case.k)
    outs = run_ranks(nranks, lambda r: fd.CEngine(n=case.n, max_cols=case.cols, gev=case.kind == "resident", rank=r, nranks=nranks),
                     lambda r, e: _gen_run(e, case, x))
    ref = _gen_reference(case, x, rows)
    for w, msgs, _ in outs:
        assert not msgs, msgs
        assert np.array_equal(w, ref), mismatch(w, ref)


# ---- 3. graded float data, componentwise bound ----------------------------------------------------------------------------------------
FLOAT_N = 769               # orders above it run at 769 (the knobs force the schedules): the long-double reference stays cheap
U32 = 2.0 ** -24
# The harness operator's entries (the polynomial form, or DAV_HARNESS_LIBM=1 the library calls on the device) against the oracle's
# host libm evaluation, relative, per entry.  Measured on MI355X at N = 513 through one-hot applies, every kernel of HARNESS below,
# with and without DAV_HARNESS_LIBM: at most 2.7 u (cos, A) and 11.3 u (sin, B), u = 2^-53, the same on every kernel.  The test
# below reads the entries back the same way and asserts the allowance before it uses it.
HARNESS_ENTRY = 16 * 2.0 ** -53


def within_gamma(w, a, x, u_entries=0.0):
    """|W - A X| <= (gamma_n (1 + u_e) + u_e) |A| |X|, rigorous for any order of summation with or without FMA; u_e: relative error
    of the operator's entries as the kernel reads them (fp32 tiles: 2^-24).  The reference is long double; |A| |X| in fp64 is
    enlarged by 1 / (1 - gamma_n) and the reference's own error bound is added.  Returns (ok, worst error / bound)."""
    n = a.shape[1]
    ref = a.astype(np.longdouble) @ x.astype(np.longdouble)
    tol = (gamma(n) * (1.0 + u_entries) + u_entries + gamma(n, 2.0 ** -64)) * (np.abs(a) @ np.abs(x)) / (1.0 - gamma(n))
    err = np.abs(w.astype(np.longdouble) - ref).astype(np.float64)
    return bool((err <= tol).all()), float(np.max(err / np.maximum(tol, np.finfo(float).tiny)))


def graded(n, k, seed):
    rng = np.random.default_rng(seed)
    d = 2.0 ** rng.integers(-20, 21, n).astype(np.float64)
    r = rng.standard_normal((n, n))
    a = np.asfortranarray(d[:, None] * (r + r.T) * d[None, :])
    return a, np.asfortranarray(rng.standard_normal((n, k)))


@pytest.mark.parametrize("name", [c.name for c in STORED])
def test_stored_operator_products_on_graded_data_are_within_gamma_n(name, monkeypatch):
    case = STORED_BY_NAME[name]
    case = case._replace(n=min(case.n, FLOAT_N))
    _set_env(monkeypatch, case.env)
    a, x = graded(case.n, case.k, _seed("graded", case.name))
    with fd.CEngine(n=case.n, max_cols=case.cols) as e:
        _set_stored(e, case, a)
        w, msgs = fenced_apply(e, x, case.c0, case.d0, case.cols, _apply_fn(e, case.inner))
    assert not msgs, msgs
    # the inner sweep reads the fp32 tiles in launches of up to 16 columns (the paired 32-column launches read the fp64 tiles)
    width = np.minimum(32, case.k - 32 * (np.arange(case.k) // 32))
    ok, worst = within_gamma(w, a, x, np.where(case.inner & (width <= 16), U32, 0.0))
    assert ok, (case.name, worst)


class HarnessCase(NamedTuple):
    name: str
    storage: int
    env: dict
    k: int
    reaches: tuple


HARNESS = [
    HarnessCase("free-harness-k9", 0, {}, 9, (free(1, 3),)),
    HarnessCase("free-harness-k17", 0, {}, 17, (free(2, 3),)),
    HarnessCase("free-harness-k40", 0, {}, 40, (free(4, 3),)),
    HarnessCase("free-harness-libm-k9", 0, {"DAV_HARNESS_LIBM": "1"}, 9, (free(1, 3),)),
    HarnessCase("sym-harness-k8", 1, {}, 8, (s8(True),)),
    HarnessCase("sym-harness-libm-k8", 1, {"DAV_HARNESS_LIBM": "1"}, 8, (s8(True),)),
    HarnessCase("sym-harness-r2-k16", 1, R2, 16, (s9(2, gen=True, harn=1), s9(2, gen=True, harn=2))),
    HarnessCase("sym-harness-r2-k40", 1, R2, 40, (sw(2, gen=2), sw(2, gen=3))),
    HarnessCase("sym-harness-r2-k24", 1, R2, 24, (sw(2, gen=2), sw(2, gen=3))),
    HarnessCase("sym-harness-r4-k8", 1, R4, 8, (s9(4, gen=True, m4=True, harn=1), s9(4, gen=True, m4=True, harn=2))),
    HarnessCase("sym-harness-libm-r2-k16", 1, {**R2, "DAV_HARNESS_LIBM": "1"}, 16, (s9(2, gen=True, harn=3),)),
    HarnessCase("sym-harness-libm-r4-k8", 1, {**R4, "DAV_HARNESS_LIBM": "1"}, 8, (s9(4, gen=True, m4=True, harn=3),)),
]
HARNESS_BY_NAME = {c.name: c for c in HARNESS}
_HARNESS_N = 513


def _entries(e, which, n, k):
    """the operator's entries as the kernels of k-column applies evaluate them: A e_j is column j exactly (every other term is 0)"""
    cols = []
    for c0 in range(0, n, k):
        kk = min(k, n - c0)
        x = np.zeros((n, kk), order="F")
        x[c0 + np.arange(kk), np.arange(kk)] = 1.0
        e.panel_put(PANEL_V, 0, x)
        e.apply(which, PANEL_V, 0, kk, PANEL_W, 0)
        cols.append(e.panel_get(PANEL_W, 0, kk))
    return np.hstack(cols)


@pytest.mark.parametrize("name", [c.name for c in GEN] + [c.name for c in HARNESS])
def test_generated_operator_products_on_graded_data_are_within_gamma_n(name, monkeypatch):
    """the hashed / generated operators bitwise equal the oracle's matrix; the harness operator's entries, read back through one-hot
    applies of the same width (A e_j is column j exactly), lie within HARNESS_ENTRY of the oracle's, and the bound allows for that"""
    n = min(GEN_BY_NAME[name].n, FLOAT_N) if name in GEN_BY_NAME else _HARNESS_N
    rng = np.random.default_rng(_seed("graded", name))
    x = np.asfortranarray(rng.standard_normal((n, 40)) * 2.0 ** rng.integers(-20, 21, n)[:, None])
    if name in GEN_BY_NAME:
        case = GEN_BY_NAME[name]._replace(n=n)
        _set_env(monkeypatch, case.env)
        x = x[:, :case.k]
        with fd.CEngine(n=n, max_cols=case.cols, gev=case.kind == "resident") as e:
            which = _set_generated(e, case)
            w, msgs = fenced_apply(e, x, case.c0, case.d0, case.cols, _apply_fn(e, which=which))
        a = O.generate_diagonal_dominant(n, SPARSITY, 1.0 if case.kind == "resident" else None, seed=SEED)
        checks = [(w, a, 0.0)]
    else:
        case = HARNESS_BY_NAME[name]
        _set_env(monkeypatch, case.env)
        x = x[:, :case.k]
        cols = case.k + 20
        with fd.CEngine(n=n, max_cols=cols, gev=True) as e:
            e.set_storage(case.storage)
            tab = O.harness_exp_table(n)
            e.set_operator_harness(OP_A, tab)
            e.set_operator_harness(OP_B, tab)
            wa, msgs = fenced_apply(e, x, 1, 3, cols, _apply_fn(e, which=OP_A))
            wb, msgs2 = fenced_apply(e, x, 3, 1, cols, _apply_fn(e, which=OP_B))
            msgs += msgs2
            entries = [_entries(e, op, n, case.k) for op in (OP_A, OP_B)]
        am, bm = O.harness_matrices(n)
        for got, ref, op in zip(entries, (am, bm), "AB"):
            dev = np.abs(got - ref) / np.abs(ref)
            assert (dev <= HARNESS_ENTRY).all(), (name, op, float(dev.max()) / 2.0 ** -53)
        checks = [(wa, am, HARNESS_ENTRY), (wb, bm, HARNESS_ENTRY)]
    assert not msgs, msgs
    for w, a, ue in checks:
        ok, worst = within_gamma(w, a, x, ue)
        assert ok, (name, worst)


# ---- 4. gram and panel_transform: exact integers, fences ----------------------------------------------------------------------------
GRAM_N = 2305               # 10 row chunks of the Gram kernels: fused finish by default, gram_reduce_kernel with DAV_GRAM_FUSE=1
GRAM_CASES = [(6, 6, 1, 3, "gram_kernel<4, 4, 4>"), (33, 17, 3, 1, "gram_kernel<8, 8, 3>"), (40, 8, 1, 1, "gram_kernel<8, 4, 4>")]


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_gram_products_are_exact_and_leave_the_panels_alone(fuse, monkeypatch):
    monkeypatch.setenv("DAV_GRAM_FUSE", fuse)           # 0: the default (fused up to 24 chunks); 1: the two-kernel route
    n, cols = GRAM_N, 64
    rng = np.random.default_rng(_seed("gram", fuse))
    with fd.CEngine(n=n, max_cols=cols) as e:
        for p, q, p0, q0, _ in GRAM_CASES:
            P = int_block(n, p, rng, bits=20)           # |P^T Q| partial sums below 2^51: exact in any order
            Q = int_block(n, q, rng, bits=20)
            sp = np.full((n, cols), np.nan, order="F")
            sp[:, p0:p0 + p] = P
            sq = np.full((n, cols), np.nan, order="F")
            sq[:, q0:q0 + q] = Q
            e.panel_put(PANEL_V, 0, sp)
            e.panel_put(PANEL_W, 0, sq)
            G = e.gram(PANEL_V, p0, p, PANEL_W, q0, q)
            assert np.array_equal(G, P.T @ Q), (p, q, mismatch(G, P.T @ Q))
            assert same_bits(e.panel_get(PANEL_V, 0, cols), sp) and same_bits(e.panel_get(PANEL_W, 0, cols), sq), (p, q)


PT_CASES = [(12, 9, 1, 3, 1), (33, 24, 3, 1, 2), (64, 40, 1, 5, 4), (20, 64, 7, 1, 4)]      # p, q, s0, d0, QT of panel_gemm_kernel


@pytest.mark.parametrize("pin", ["1", "0"])
def test_panel_transform_is_exact_and_fenced(pin, monkeypatch):
    monkeypatch.setenv("DAV_PG_PIN", pin)
    n, cols = GRAM_N, 96
    rng = np.random.default_rng(_seed("transform", pin))
    with fd.CEngine(n=n, max_cols=cols) as e:
        for p, q, s0, d0, _ in PT_CASES:
            for P, M in ((int_block(n, p, rng), rng.integers(-255, 256, (p, q)).astype(np.float64)),
                         (unit_block(n, p, rng), rng.integers(-4, 5, (p, q)).astype(np.float64))):
                src = np.full((n, cols), np.nan, order="F")
                src[:, s0:s0 + p] = P
                e.panel_put(PANEL_V, 0, src)
                e.panel_put(PANEL_W, 0, np.full((n, cols), SENTINEL, order="F"))
                e.panel_transform(PANEL_V, s0, p, M, PANEL_W, d0)
                w = e.panel_get(PANEL_W, 0, cols)
                assert same_bits(e.panel_get(PANEL_V, 0, cols), src), (p, q)
                outside = np.ones(cols, dtype=bool)
                outside[d0:d0 + q] = False
                assert (w[:, outside] == SENTINEL).all(), (p, q)
                ref = exact_dense_product(M.T, P.T).T
                assert np.array_equal(w[:, d0:d0 + q], ref), (p, q, mismatch(w[:, d0:d0 + q], ref))
            assert gram_is_exact(e.gram(PANEL_W, d0, q, PANEL_W, d0, q), w[:, d0:d0 + q]), (p, q)


# ---- 5. CSR and BSR: structural NaN, chunk edges ------------------------------------------------------------------------------------
SP_COLS = 120
CSR_N = 3000
CSR_LONG = {2990: 1024, 2991: 1025, 2992: 2048, 2993: 2049}      # CSR_CHUNK = 1024: one item; 2, 2 and 3 chunks
CSR_ONLY_LONG = np.arange(2900, 2990)                            # rows that only the long rows (and their own diagonal) read
CSR_KS = [(1, 0, 0), (17, 1, 3), (24, 1, 1), (33, 3, 1), (63, 3, 5), (96, 5, 7)]


def csr_matrix():
    """symmetric integer CSR: short rows (about 8 entries, runs of CSR_ROWS = 16 rows per work item) with explicit zeros and
    duplicates, and long rows of exactly 1024, 1025, 2048 and 2049 entries (duplicates among them)"""
    rng = np.random.default_rng(_seed("csr"))
    n = CSR_N
    longs = np.array(sorted(CSR_LONG))
    short = np.setdiff1d(np.arange(n), np.concatenate([longs, CSR_ONLY_LONG]))
    i = np.repeat(short, 3)
    j = rng.choice(short, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    v = rng.integers(-255, 256, i.size)
    v[::13] = 0
    dup = np.arange(0, i.size, 11)
    rows = [np.arange(n), i, j, i[dup], j[dup]]
    cols = [np.arange(n), j, i, j[dup], i[dup]]
    vals = [rng.integers(1, 256, n), v, v, v[dup], v[dup]]
    pool = np.concatenate([short, CSR_ONLY_LONG])
    for L, T in CSR_LONG.items():
        c = rng.choice(pool, T - 1)
        w = rng.integers(-255, 256, T - 1)
        rows += [np.full(T - 1, L), c]
        cols += [c, np.full(T - 1, L)]
        vals += [w, w]
    rows, cols, vals = (np.concatenate(z) for z in (rows, cols, vals))
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order].astype(np.float64)
    indptr = np.searchsorted(rows, np.arange(n + 1)).astype(np.int64)
    assert all(indptr[L + 1] - indptr[L] == T for L, T in CSR_LONG.items())
    return indptr, rows, cols, vals


def _csr_nan_rows():
    return np.array([0, CSR_ONLY_LONG[0], CSR_ONLY_LONG[7], 1234])


def _sparse_inputs(n, nan_rows, tag):
    rng = np.random.default_rng(_seed("sparse X", tag))
    x = int_block(n, 96, rng)
    x[nan_rows] = np.nan
    return x, unit_block(n, 96, rng)


def _sparse_run(e, ks, x, xs):
    ap = _apply_fn(e)
    out = []
    for k, c0, d0 in ks:
        w, msgs = fenced_apply(e, x[:, :k], c0, d0, SP_COLS, ap, stale=k + 16)
        ws, msgs2 = fenced_apply(e, xs[:, :k], c0, d0, SP_COLS, ap)
        out.append((w, msgs + msgs2, ws, e.gram(PANEL_W, d0, k, PANEL_W, d0, k)))
    return out


def _check_sparse(tag, ks, out, ref, refs, hit):
    assert 0 < hit.sum() < hit.size // 4            # the design: a few rows read a NaN, most do not
    for (k, c0, d0), (w, msgs, ws, g) in zip(ks, out):
        assert not msgs, (tag, k, msgs)
        assert np.isnan(w[hit]).all(), (tag, k, "rows that read a NaN row of X are finite")
        assert np.array_equal(w[~hit], ref[~hit, :k]), (tag, k, mismatch(w[~hit], ref[~hit, :k]))
        assert np.array_equal(ws, refs[:, :k]), (tag, k, mismatch(ws, refs[:, :k]))
        assert gram_is_exact(g, ws), (tag, k, "padding rows of the result are not zero")


def test_csr_products_are_exact_with_nan_exactly_where_the_pattern_reads_one():
    indptr, rows, cols, vals = csr_matrix()
    nan_rows = _csr_nan_rows()
    x, xs = _sparse_inputs(CSR_N, nan_rows, "csr")
    with fd.CEngine(n=CSR_N, max_cols=SP_COLS) as e:
        e.set_operator_csr(OP_A, indptr, cols, vals)
        out = _sparse_run(e, CSR_KS, x, xs)
    _check_sparse("csr", CSR_KS, out, exact_sparse_product(CSR_N, rows, cols, vals, x),
                  exact_sparse_product(CSR_N, rows, cols, vals, xs), touched_rows(CSR_N, rows, cols, nan_rows))


@pytest.mark.parametrize("nranks", [2, 3, 5])
def test_csr_products_are_exact_over_ranks(nranks):
    indptr, rows, cols, vals = csr_matrix()
    nan_rows = _csr_nan_rows()
    x, xs = _sparse_inputs(CSR_N, nan_rows, "csr")

    def work(r, e):
        e.set_operator_csr(OP_A, indptr, cols, vals)
        return _sparse_run(e, CSR_KS, x, xs)
    outs = run_ranks(nranks, lambda r: fd.CEngine(n=CSR_N, max_cols=SP_COLS, rank=r, nranks=nranks), work)
    ref, refs = exact_sparse_product(CSR_N, rows, cols, vals, x), exact_sparse_product(CSR_N, rows, cols, vals, xs)
    hit = touched_rows(CSR_N, rows, cols, nan_rows)
    for out in outs:
        _check_sparse(f"csr {nranks} ranks", CSR_KS, out, ref, refs, hit)


BSR_NB = 260
BSR_LONG = {257: 128, 258: 129, 259: 256}                        # BSR_CHUNK = 128 blocks: one item; 2 and 2 chunks
BSR_ONLY_LONG = np.arange(240, 257)
# 1 column group; 2 (the second partly filled); 3 promoted to 4; 4 with a partly filled last; 4 then 2 (the second launch at column 64)
BSR_KS = [(9, 1, 3), (24, 5, 3), (40, 1, 1), (63, 3, 5), (96, 3, 1)]


def bsr_matrix(b):
    """symmetric integer BSR with b x b blocks: short block rows (diagonal block and about four more, explicit zero blocks,
    duplicates) and long block rows of exactly 128, 129 and 256 blocks"""
    rng = np.random.default_rng(_seed("bsr", b))
    nb = BSR_NB
    longs = np.array(sorted(BSR_LONG))
    short = np.setdiff1d(np.arange(nb), np.concatenate([longs, BSR_ONLY_LONG]))

    def blocks(m):
        return rng.integers(-255, 256, (m, b, b))

    d = blocks(nb)
    d = np.tril(d) + np.swapaxes(np.tril(d, -1), 1, 2)
    i = np.repeat(short, 2)
    j = rng.choice(short, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    w = blocks(i.size)
    w[::9] = 0
    dup = np.arange(0, i.size, 7)
    bi = [np.arange(nb), i, j, i[dup], j[dup]]
    bj = [np.arange(nb), j, i, j[dup], i[dup]]
    bv = [d, w, np.swapaxes(w, 1, 2), w[dup], np.swapaxes(w[dup], 1, 2)]
    pool = np.concatenate([short, BSR_ONLY_LONG])
    for L, T in BSR_LONG.items():
        c = rng.choice(pool, T - 1)
        wl = blocks(T - 1)
        bi += [np.full(T - 1, L), c]
        bj += [c, np.full(T - 1, L)]
        bv += [wl, np.swapaxes(wl, 1, 2)]
    bi, bj, bv = (np.concatenate(z) for z in (bi, bj, bv))
    order = np.argsort(bi, kind="stable")
    bi, bj, bv = bi[order], bj[order], np.ascontiguousarray(bv[order], dtype=np.float64)
    indptr = np.searchsorted(bi, np.arange(nb + 1)).astype(np.int64)
    assert all(indptr[L + 1] - indptr[L] == T for L, T in BSR_LONG.items())
    return indptr, bi, bj, bv


def _bsr_nan_rows(b):
    """row 0; the first row of a block column (for b not a multiple of 4: inside the previous block column's padded K-steps); a row
    of a block column that only the long block rows read"""
    return np.array([0, 11 * b, BSR_ONLY_LONG[0] * b + b - 1])


def bsr_product(b, bi, bj, bv, x):
    k = x.shape[1]
    xi = np.where(np.isnan(x), 0.0, x).astype(np.int64).reshape(BSR_NB, b, k)
    t = np.einsum("pmq,pqc->pmc", bv.astype(np.int64), xi[bj])
    y = np.zeros((BSR_NB, b, k), dtype=np.int64)
    np.add.at(y, bi, t)
    return y.reshape(BSR_NB * b, k).astype(np.float64)


def bsr_touched(b, bi, bj, nan_rows):
    bad = np.zeros(BSR_NB, dtype=bool)
    bad[np.asarray(nan_rows) // b] = True
    hit = np.zeros(BSR_NB, dtype=bool)
    np.logical_or.at(hit, bi, bad[bj])
    return np.repeat(hit, b)


def _bsr_case(b):
    indptr, bi, bj, bv = bsr_matrix(b)
    n = BSR_NB * b
    nan_rows = _bsr_nan_rows(b)
    x, xs = _sparse_inputs(n, nan_rows, ("bsr", b))
    return n, indptr, bi, bj, bv, x, xs, (bsr_product(b, bi, bj, bv, x), bsr_product(b, bi, bj, bv, xs), bsr_touched(b, bi, bj, nan_rows))


@pytest.mark.parametrize("b", [1, 3, 5, 7, 8, 9, 16])
def test_bsr_products_are_exact_with_nan_exactly_where_the_pattern_reads_one(b):
    n, indptr, bi, bj, bv, x, xs, (ref, refs, hit) = _bsr_case(b)
    with fd.CEngine(n=n, max_cols=SP_COLS) as e:
        e.set_operator_bsr(OP_A, indptr, bj.astype(np.int32), bv)
        out = _sparse_run(e, BSR_KS, x, xs)
    _check_sparse(f"bsr b={b}", BSR_KS, out, ref, refs, hit)


# three ranks: slabs of 260 b / 3 rows - block rows straddle two slabs for b = 3, 7, 9 (and 16: 1387 rows); 2 and 5 ranks at b = 5
@pytest.mark.parametrize("b,nranks", [(3, 3), (7, 3), (9, 3), (16, 3), (5, 2), (5, 5)])
def test_bsr_products_are_exact_over_ranks(b, nranks):
    n, indptr, bi, bj, bv, x, xs, (ref, refs, hit) = _bsr_case(b)

    def work(r, e):
        e.set_operator_bsr(OP_A, indptr, bj.astype(np.int32), bv)
        return _sparse_run(e, BSR_KS, x, xs)
    outs = run_ranks(nranks, lambda r: fd.CEngine(n=n, max_cols=SP_COLS, rank=r, nranks=nranks), work)
    for out in outs:
        _check_sparse(f"bsr b={b} {nranks} ranks", BSR_KS, out, ref, refs, hit)


# ---- 7. dispatch table ------------------------------------------------------------------------------------------------------------------
def _dispatch():
    table = {}
    for case in STORED + GEN + HARNESS:
        for inst in case.reaches:
            table.setdefault(inst, []).append(case.name)
    for g in (1, 2, 4):
        table[f"spmm_csr_kernel<{g}>"] = ["csr k=1" if g == 1 else "csr k=17 / 24 / 96" if g == 2 else "csr k=33 / 63 / 96"]
    table["spmm_csr_finish_kernel"] = ["csr rows of 1025, 2048, 2049 entries"]
    for ns, bs in ((1, "b=1, 3"), (2, "b=5, 7, 8"), (3, "b=9"), (4, "b=16")):
        for gp, ks in ((1, "k=9"), (2, "k=24, 96 (columns 64-95)"), (4, "k=40 (3 groups -> 4), 63, 96 (columns 0-63)")):
            table[f"spmm_bsr_kernel<{ns}, {_b(ns >= 3)}, {gp}>"] = [f"bsr {bs}, {ks}"]
    table["spmm_bsr_finish_kernel"] = ["bsr block rows of 129 and 256 blocks"]
    for p, q, _, _, inst in GRAM_CASES:
        table[inst] = [f"gram {p} x {q}"]
    table["gram_reduce_kernel"] = ["gram, DAV_GRAM_FUSE=1"]
    for qt in (1, 2, 4):
        for pin in (True, False):
            table[f"panel_gemm_kernel<{qt}, 8, {_b(pin)}>"] = [f"panel_transform QT={qt}, DAV_PG_PIN={int(pin)}"]
    table["pack_xt_kernel"] = ["every apply"]
    table["chunk_to_panel_kernel"] = ["every case over ranks (the rows of the reduce-scatter into the panel)"]
    table["zero_pad_rows_kernel"] = ["csr, bsr (the padding rows of the result)"]
    return table


DISPATCH = _dispatch()

# Instantiations of the block-product kernels that no case reaches through the C ABI, and why.  Every other instantiation compiled
# into the library is in DISPATCH: the dense-tile kernel templates are instantiated only by the launch branches listed above.
UNREACHABLE = {}
