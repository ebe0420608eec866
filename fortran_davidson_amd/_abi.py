"""The C ABI as ctypes sees it: one prototype per entry point, name -> (restype, argtypes), applied to a library once when it is loaded
(_lib.py).  Scalars carry their exact type, so a call that passes a scalar wrapped in another type raises ctypes.ArgumentError instead
of handing the callee the wrong width, and a plain Python int or float is converted to the declared one.  Everything passed as an
address - data pointers, dav_handle_t and dav_handle_t*, const char*, dav_device_apply_fn, type(c_ptr) / type(c_funptr) values, Fortran
array and intent(out) dummies - is c_void_p, which takes byref(), data_as() pointers, ctypes arrays and buffers, bytes, None, ints and
function pointers alike.  tests/test_abi_cpu.py compares both tables with the headers and the Fortran sources."""
import ctypes as C

i32, i64, u64, size, f64, ptr = C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_double, C.c_void_p

# include/davidson_hip.h, then csrc/davidson_hip_private.h, in the headers' order
DAV = {
    "dav_last_error": (C.c_char_p, ()),
    "dav_version": (i32, ()),
    "dav_create": (i32, (ptr, i32, i64, i32, i32, i32, i32)),
    "dav_destroy": (i32, (ptr,)),
    "dav_comm_unique_id": (i32, (ptr,)),
    "dav_comm_init": (i32, (ptr, ptr)),
    "dav_comm_path": (i32, (ptr, ptr, ptr, ptr, ptr, ptr)),
    "dav_synchronize": (i32, (ptr,)),
    "dav_get_stats": (i32, (ptr, ptr)),
    "dav_get_stats_n": (i32, (ptr, ptr, size)),
    "dav_reset_stats": (i32, (ptr,)),
    "dav_set_timing": (i32, (ptr, i32)),
    "dav_local_rows": (i32, (ptr, ptr, ptr)),
    "dav_set_storage": (i32, (ptr, i32)),
    "dav_device_memory": (i32, (ptr, ptr, ptr)),
    "dav_free_buffers": (i32, ()),
    "dav_set_dense_host": (i32, (ptr, i32, ptr, i64)),
    "dav_set_dense_dev": (i32, (ptr, i32, ptr, i64)),
    "dav_dense_begin": (i32, (ptr, i32)),
    "dav_dense_put_rows": (i32, (ptr, i32, i64, i64, ptr, i64)),
    "dav_dense_end": (i32, (ptr, i32)),
    "dav_set_dense_file": (i32, (ptr, i32, ptr, i32)),
    "dav_parse_text_f64": (i32, (ptr, size, ptr, size, ptr)),
    "dav_set_dense_generated": (i32, (ptr, i32, u64, f64, i32, f64)),
    "dav_set_operator_hashed": (i32, (ptr, i32, u64, f64, i32, f64)),
    "dav_set_operator_harness": (i32, (ptr, i32, ptr)),
    "dav_set_operator_identity": (i32, (ptr, i32)),
    "dav_set_operator_host": (i32, (ptr, i32, ptr)),
    "dav_set_operator_device": (i32, (ptr, i32, ptr, ptr, ptr)),
    "dav_set_operator_csr": (i32, (ptr, i32, ptr, ptr, ptr, i32, i32)),
    "dav_set_operator_csr_dev": (i32, (ptr, i32, ptr, i32, ptr, i32, ptr, i32, i32)),
    "dav_set_operator_bsr": (i32, (ptr, i32, i32, ptr, ptr, ptr, i32, i32, i32)),
    "dav_set_operator_bsr_dev": (i32, (ptr, i32, i32, ptr, i32, ptr, i32, ptr, i32, i32, i32)),
    "dav_keep_value_map": (i32, (ptr, i32, i32)),
    "dav_update_operator_values": (i32, (ptr, i32, ptr)),
    "dav_update_operator_values_dev": (i32, (ptr, i32, ptr)),
    "dav_get_diagonal": (i32, (ptr, i32, ptr)),
    "dav_init_basis": (i32, (ptr, i32, ptr)),
    "dav_set_guess": (i32, (ptr, ptr, i64, i32)),
    "dav_set_guess_dev": (i32, (ptr, ptr, i64, i32)),
    "dav_keep_result_as_guess": (i32, (ptr, i32)),
    "dav_mark_result_as_guess": (i32, (ptr, i32)),
    "dav_guess_columns": (i32, (ptr, ptr)),
    "dav_init_basis_guess": (i32, (ptr, i32, ptr, ptr)),
    "dav_apply": (i32, (ptr, i32, i32, i32, i32, i32, i32)),
    "dav_gram": (i32, (ptr, i32, i32, i32, i32, i32, i32, ptr, i64)),
    "dav_project": (i32, (ptr, i32, i32, ptr, i64, ptr, i64)),
    "dav_ritz_residual_correction": (i32, (ptr, i32, i32, ptr, i64, ptr, i32, ptr)),
    "dav_ritz_residual_correction_n": (i32, (ptr, i32, i32, i32, ptr, i64, ptr, i32, ptr)),
    "dav_panel_select": (i32, (ptr, i32, i32, i32, ptr)),
    "dav_ritz_residual_correction_g": (i32, (ptr, i32, i32, i32, ptr, i64, ptr, ptr, ptr, i64, ptr, i64)),
    "dav_set_lazy_ritz_vectors": (i32, (ptr, i32)),
    "dav_ritz_vectors": (i32, (ptr, i32, i32, ptr, i64)),
    "dav_gjd_correction": (i32, (ptr, i32, ptr, i32, f64, ptr)),
    "dav_gjd_correction_n": (i32, (ptr, i32, i32, ptr, i32, f64, ptr, ptr)),
    "dav_ortho_gram": (i32, (ptr, i32, i32, ptr, i64, ptr, i64)),
    "dav_ortho_apply": (i32, (ptr, i32, i32, ptr, i64, ptr, i64)),
    "dav_project_ortho": (i32, (ptr, i32, i32, ptr, i64, ptr, i64, ptr, i64, ptr, i64)),
    "dav_ortho_apply_all": (i32, (ptr, i32, i32, ptr, i64, ptr, i64)),
    "dav_expand": (i32, (ptr, i32, i32)),
    "dav_restart": (i32, (ptr, i32, i32, ptr, i64)),
    "dav_ranks_agree": (i32, (ptr, ptr, i32)),
    "dav_agree_next": (i32, (ptr, ptr, i32)),
    "dav_agree_inputs": (i32, (ptr, ptr, i32)),
    "dav_set_inner_precision": (i32, (ptr, i32)),
    "dav_rr_enable": (i32, (ptr, i32)),
    "dav_project_dev": (i32, (ptr, i32, i32)),
    "dav_rr_ritz": (i32, (ptr, i32, i32, i32, i32, ptr, ptr, ptr, i64, ptr, i64, ptr)),
    "dav_rr_restart": (i32, (ptr, i32, i32)),
    "dav_rr_get": (i32, (ptr, i32, i32, ptr, ptr, i64)),
    "dav_panel_transform": (i32, (ptr, i32, i32, i32, ptr, i64, i32, i32, i32)),
    "dav_panel_get": (i32, (ptr, i32, i32, i32, ptr, i64)),
    "dav_panel_put": (i32, (ptr, i32, i32, i32, ptr, i64)),
    "dav_panel_unit_column": (i32, (ptr, i32, i32, i32)),
    "dav_set_width": (i32, (ptr, i32)),

    "dav_bench_apply": (i32, (ptr, i32, i32, i32, ptr, ptr)),
    "dav_bench_apply2": (i32, (ptr, i32, i32, i32, ptr, ptr, ptr, ptr)),
    "dav_bench_stream": (i32, (ptr, i64, i32, ptr, ptr)),
    "dav_bench_stream3": (i32, (ptr, i64, i32, ptr, ptr, ptr)),
    "dav_bench_harness_rate": (i32, (ptr, i32, ptr)),
    "dav_apply_inner": (i32, (ptr, i32, i32, i32, i32, i32, i32)),
    "dav_resident_fraction": (i32, (ptr, i32, ptr)),
    "dav_buffer_cache_held": (i32, (ptr, ptr)),
    "dav_pack_operand_image": (i32, (ptr, i64, i32, i32, ptr, ptr, ptr)),
    "dav_local_group_join": (i32, (ptr, i32)),
    "dav_local_group_yield": (i32, (ptr,)),
    "dav_comm_init_shm": (i32, (ptr, ptr)),
}

# entries of the private header that only lib/test/libdavidson_hip.so (-DDAV_TEST_TRANSPORTS=1) exports
TEST_BUILD_ONLY = ("dav_local_group_join", "dav_local_group_yield", "dav_comm_init_shm")

# the bind(C) doors of fortran/davidson_c_api.f90, in the source's order (None: a subroutine)
FD = {
    "fd_dense_solve": (None, (i32, ptr, i32, ptr, i32, i32, i32, f64, i32, ptr, ptr, ptr)),
    "fd_sparse_solve": (None, (i32, ptr, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32, i32, i32, f64, i32, ptr, ptr, ptr)),
    "fd_bsr_solve": (None, (i32, i32, ptr, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32, i32, i32, f64, i32, ptr, ptr, ptr)),
    "fd_free_solve": (None, (i32, ptr, ptr, i32, i32, f64, i32, ptr, ptr, ptr)),
    "fd_engine_create": (ptr, (i32, i32, i32, i32, i32, i32, i32)),
    "fd_engine_destroy": (None, (ptr,)),
    "fd_engine_handle": (ptr, (ptr,)),
    "fd_engine_comm_unique_id": (None, (ptr,)),
    "fd_engine_comm_init": (None, (ptr, ptr)),
    "fd_engine_set_storage": (None, (ptr, i32)),
    "fd_engine_set_inner_precision": (None, (ptr, i32)),
    "fd_engine_set_device_rr": (None, (ptr, i32)),
    "fd_engine_set_policy": (None, (ptr, i32)),
    "fd_engine_set_dense": (None, (ptr, i32, ptr)),
    "fd_engine_set_sparse": (None, (ptr, i32, i32, ptr, ptr, ptr, i32, i32)),
    "fd_engine_set_sparse_device": (i32, (ptr, i32, i32, ptr, i32, ptr, i32, ptr, i32, i32)),
    "fd_engine_set_block_sparse": (None, (ptr, i32, i32, i32, ptr, ptr, ptr, i32, i32)),
    "fd_engine_set_block_sparse_device": (i32, (ptr, i32, i32, i32, ptr, i32, ptr, i32, ptr, i32, i32, i32)),
    "fd_engine_keep_value_map": (None, (ptr, i32, i32)),
    "fd_engine_update_values": (None, (ptr, i32, ptr, i64)),
    "fd_engine_update_values_device": (i32, (ptr, i32, ptr)),
    "fd_engine_set_initial_vectors": (i32, (ptr, ptr, i32)),
    "fd_engine_set_initial_vectors_device": (i32, (ptr, ptr, i32, i32)),
    "fd_engine_keep_result_as_guess": (None, (ptr, i32)),
    "fd_dense_solve_guess": (None, (i32, ptr, i32, ptr, i32, i32, i32, f64, i32, i32, ptr, ptr, ptr, ptr)),
    "fd_sparse_solve_guess": (None, (i32, ptr, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32, i32, i32, f64, i32, i32, ptr, ptr, ptr, ptr)),
    "fd_bsr_solve_guess": (None, (i32, i32, ptr, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32, i32, i32, f64, i32, i32, ptr, ptr, ptr, ptr)),
    "fd_free_solve_guess": (None, (i32, ptr, ptr, i32, i32, f64, i32, i32, ptr, ptr, ptr, ptr)),
    "fd_engine_set_operator": (None, (ptr, i32, i32, i32, f64, i32, f64)),
    "fd_engine_solve": (None, (ptr, i32, i32, i32, f64, i32, ptr, i32, ptr, ptr)),
    "fd_engine_phase_seconds": (None, (ptr, ptr)),
    "fd_engine_fits_as_full_rows": (i32, (ptr, i32, i32)),
    "fd_lapack_eigensolver": (None, (i32, ptr, i32, ptr, ptr, ptr)),
    "fd_lapack_rayleigh_ritz": (None, (i32, ptr, i32, ptr, i32, ptr, ptr)),
    "fd_lapack_qr": (None, (i32, i32, ptr)),
    "fd_lapack_solver": (None, (i32, ptr, ptr)),
    "fd_lapack_matmul": (None, (i32, i32, i32, i32, i32, ptr, ptr, ptr)),
    "fd_lapack_sort": (None, (i32, i32, ptr, ptr)),
    "fd_generate_preconditioner": (None, (i32, ptr, i32, ptr)),
    "fd_generate_diagonal_dominant": (None, (i32, f64, i32, f64, i32, ptr)),
    "fd_norm": (None, (i32, ptr, ptr)),
}

# include/davidson_hip_ext.h: the extension entries (prefix davx_) next to ABI 109, and their doors (prefix fdx_) of davidson_c_api.f90;
# tests/test_coo_cpu.py compares both with the header and the Fortran sources, as tests/test_abi_cpu.py does for the tables above
EXT = {
    "davx_set_operator_coo": (i32, (ptr, i32, i64, ptr, ptr, ptr, i32, i32)),
    "davx_set_operator_coo_dev": (i32, (ptr, i32, i64, ptr, i32, ptr, i32, ptr, i32, i32)),
}
EXT_FD = {
    "fdx_engine_set_coo": (None, (ptr, i32, i32, i64, ptr, ptr, ptr, i32, i32)),
    "fdx_engine_set_coo_device": (i32, (ptr, i32, i32, i64, ptr, i32, ptr, i32, ptr, i32, i32)),
}

# include/davidson_hip_herm.h: complex Hermitian CSR operators through their real form (prefix davh_) and their doors (prefix fdh_);
# tests/test_herm_cpu.py compares both with the header and the Fortran sources
HERM = {
    "davh_set_operator_csr": (i32, (ptr, i32, ptr, ptr, ptr, i32, i32)),
    "davh_set_operator_csr_dev": (i32, (ptr, i32, ptr, i32, ptr, i32, ptr, i32, i32)),
}
HERM_FD = {
    "fdh_engine_set_hermitian": (None, (ptr, i32, i32, ptr, ptr, ptr, i32, i32)),
    "fdh_engine_set_hermitian_device": (i32, (ptr, i32, i32, ptr, i32, ptr, i32, ptr, i32, i32)),
}

# include/davidson_hip_precond.h: the preconditioner the engine builds from the stored operators (prefix davp_) and its doors (prefix
# fdp_); tests/test_fsai_cpu.py compares both with the header and the Fortran sources
PRECOND = {
    "davp_build_fsai": (i32, (ptr, f64, i32)),
    "davp_fsai_info": (i32, (ptr, ptr, ptr, ptr)),
    "davp_fsai_get_factor": (i32, (ptr, i32, ptr, ptr, ptr)),
}
PRECOND_FD = {
    "fdp_engine_build_fsai": (i32, (ptr, f64, i32)),
    "fdp_engine_fsai_info": (None, (ptr, ptr, ptr, ptr)),
}

# include/davidson_hip_bprecond.h: the block preconditioner the engine builds from stored BSR operators (prefix davq_) and its doors
# (prefix fdq_); tests/test_bfsai_cpu.py compares both with the header and the Fortran sources
BPRECOND = {
    "davq_build_block_fsai": (i32, (ptr, f64, i32)),
    "davq_block_fsai_info": (i32, (ptr, ptr, ptr, ptr, ptr)),
    "davq_block_fsai_get_factor": (i32, (ptr, i32, ptr, ptr, ptr)),
}
BPRECOND_FD = {
    "fdq_engine_build_block_fsai": (i32, (ptr, f64, i32)),
    "fdq_engine_block_fsai_info": (None, (ptr, ptr, ptr, ptr, ptr)),
}


def apply(lib, table, optional=()):
    """Set restype and argtypes of every entry of `table` on `lib`.  An entry of `optional` that the library lacks is skipped; any
    other missing symbol is an error: the library is not the one these tables describe."""
    missing = []
    for name, (restype, argtypes) in table.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if name not in optional:
                missing.append(name)
            continue
        fn.restype, fn.argtypes = restype, argtypes
    if missing:
        raise RuntimeError(f"{lib._name} does not export {', '.join(missing)}: it was built from other sources than this package "
                           "(run `make -C fortran_davidson_amd`)")
