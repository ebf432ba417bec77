"""dune_ddm_amd -- MI355X-native two-level additive Schwarz + GenEO hot path (host-side mirror).

The compute lives in ``libddm_hip.so`` (hand-written HIP for gfx950, C ABI in include/ddm_hip.h).
This package is the thin host layer used by the tests and bench.py: ctypes bindings with the
reference's class names (SchwarzPreconditioner, GalerkinPreconditioner, CombinedPreconditioner,
NonOverlappingOperator), the flattening of DUNE-style index sets into exchange plans, and the
synthetic problem generator.  There is no CPU fallback: importing works anywhere (so that the
symbol table can be checked), every compute call needs a HIP device.

The directory name contains a hyphen, so import it through ``__graft_entry__.import_package()``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libddm_hip.so")

GENEO_AVAILABLE = True   # dune-ddm_amd/geneo.py: device GenEO coarse-basis builder

DDM_OK, DDM_EINVAL, DDM_EHIP, DDM_ENOTIMPL, DDM_ENUMERIC, DDM_ECOMM = 0, -1, -2, -3, -4, -5
MULTI_ENGINES = ("levels", "xcd", "xcd1")   # modes of ddm_ilu0_set_multi_engine: one launch per level; one persistent launch; that with one team


class DdmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ddm_hip error {code}: {msg}")
        self.code = code


class SolveResult(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("converged", ctypes.c_int32), ("def0", ctypes.c_double),
                ("reduction", ctypes.c_double), ("elapsed_s", ctypes.c_double)]


class GeneoParams(ctypes.Structure):
    """ddm_geneo_params: the keys of `<prefix>.eigensolver` (dune/ddm/eigensolvers/eigensolver_params.hh:8-62)"""
    _fields_ = [("nev", ctypes.c_int32), ("nev_max", ctypes.c_int32), ("tolerance", ctypes.c_double), ("shift", ctypes.c_double),
                ("threshold", ctypes.c_double), ("maxit", ctypes.c_int32), ("extra", ctypes.c_int32), ("seed", ctypes.c_int32),
                ("preconditioner", ctypes.c_int32), ("max_direct_flops", ctypes.c_double), ("verbose", ctypes.c_int32), ("raw", ctypes.c_int32)]


class GeneoInfo(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("converged", ctypes.c_int32), ("used_direct", ctypes.c_int32), ("nev", ctypes.c_int32),
                ("worst_residual", ctypes.c_double), ("setup_s", ctypes.c_double), ("iterate_s", ctypes.c_double), ("direct_flops", ctypes.c_double)]


A2A_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)

_P, _I64, _I32, _D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_PP = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); must list every symbol declared in include/ddm_hip.h
SYMBOLS = {
    "ddm_ctx_create": (_I32, [_I32, _P, _PP]),
    "ddm_ctx_destroy": (None, [_P]),
    "ddm_last_error": (ctypes.c_char_p, [_P]),
    "ddm_ctx_sync": (_I32, [_P]),
    "ddm_ctx_fence": (_I32, [_P]),
    "ddm_ctx_stream": (_P, [_P]),
    "ddm_ctx_set_comm": (_I32, [_P, _I32, _I32, A2A_FN, ALLREDUCE_FN, _P]),
    "ddm_rccl_unique_id": (_I32, [_P]),
    "ddm_ctx_set_rccl": (_I32, [_P, _I32, _I32, _P, _I32]),
    "ddm_ctx_rccl_size": (_I32, [_P, ctypes.POINTER(ctypes.c_int)]),
    "ddm_ctx_comm_counts": (_I32, [_P, _P]),
    "ddm_malloc": (_I32, [_P, _I64, _PP]),
    "ddm_free": (_I32, [_P, _P]),
    "ddm_memset_zero": (_I32, [_P, _P, _I64]),
    "ddm_memcpy_h2d": (_I32, [_P, _P, _P, _I64]),
    "ddm_memcpy_d2h": (_I32, [_P, _P, _P, _I64]),
    "ddm_csr_create": (_I32, [_P, _I64, _I64, _P, _P, _P, _PP]),
    "ddm_csr_create_host": (_I32, [_P, _I64, _I64, _P, _P, _P, _PP]),
    "ddm_csr_set_values": (_I32, [_P, _P, _P]),
    "ddm_ilu0_refresh": (_I32, [_P, _P]),
    "ddm_ilu0_refresh_count": (_I32, [_P]),
    "ddm_schwarz_refresh": (_I32, [_P, _P]),
    "ddm_op_refresh": (_I32, [_P, _P]),
    "ddm_galerkin_set_inverse": (_I32, [_P, _P, _P]),
    "ddm_csr_destroy": (None, [_P]),
    "ddm_csr_rows": (_I64, [_P]),
    "ddm_csr_nnz": (_I64, [_P]),
    "ddm_csr_mv": (_I32, [_P, _P, _P, _P]),
    "ddm_csr_usmv": (_I32, [_P, _P, _D, _P, _P]),
    "ddm_csr_mm": (_I32, [_P, _P, _I32, _P, _P]),
    "ddm_csr_row_order_tiled_host": (_I32, [_I64, _P, _P, _P, _P]),
    "ddm_dia_build_and_apply_host": (_I32, [_I64, _P, _P, _P, _P, _P, _I64, _P, _P]),
    "ddm_dia_windows_host": (_I32, [_I64, _P, _P, _P, _I64, _P, _I64, _P, _P]),
    "ddm_dia_codes_host": (_I32, [_I64, _P, _P, _P, _I32, _I64, _P, _P, _P, _P]),
    "ddm_ilu0_solve_multi": (_I32, [_P, _P, _I32, _P, _P]),
    "ddm_ilu0_solve_multi_f32": (_I32, [_P, _P, _I32, _P, _P]),
    "ddm_ilu0_create": (_I32, [_P, _P, _I64, _P, _PP]),
    "ddm_ilu0_destroy": (None, [_P]),
    "ddm_ilu0_solve": (_I32, [_P, _P, _P, _P]),
    "ddm_ilu0_debug_stamps": (_I32, [_P, _P, _P, _P, _P]),
    "ddm_ilu0_status": (_I32, [_P, _P, ctypes.POINTER(ctypes.c_int)]),
    "ddm_ilu0_peek_status": (_I32, [_P]),
    "ddm_ilu0_set_status": (_I32, [_P, _I32]),
    "ddm_halo_exchange_to": (_I32, [_P, _P, _P, _P]),
    "ddm_schwarz_local_solver": (_P, [_P]),
    "ddm_ilu0_pipe_trace": (_I32, [_P, _P, _P, _P, _P, _P, _I64, ctypes.POINTER(ctypes.c_int64)]),
    "ddm_ilu0_pipe_info": (_I32, [_P, _P, _P, _I64, ctypes.POINTER(ctypes.c_int64)]),
    "ddm_ilu0_num_levels": (_I64, [_P, _I32]),
    "ddm_ilu0_wait": (_I32, [_P, _P]),
    "ddm_ilu0_box_check": (_I32, [_P, _P]),
    "ddm_ilu0_box_info": (_I32, [_P, _P, ctypes.c_int64, _P]),
    "ddm_ilu0_solve_tail": (_I32, [_P, _P, _P, _P, _P, _P]),
    "ddm_ilu0_engine": (_I32, [_P]),
    "ddm_chol_create": (_I32, [_P, _P, _I64, _P, _D, _PP]),
    "ddm_ilu0_is_direct": (_I32, [_P]),
    "ddm_ilu0_refinement": (_I32, [_P, _P]),
    "ddm_ilu0_sn_pivots": (_I32, [_P, _P, _P]),
    "ddm_sn_host_create": (_I32, [_I64, _P, _P, _I64, _P, _PP]),
    "ddm_sn_host_destroy": (None, [_P]),
    "ddm_sn_host_sizes": (_I32, [_P, _I64, _P, ctypes.POINTER(ctypes.c_double)]),
    "ddm_sn_host_get": (_I32, [_P, _I64, _P, _P, _P, _P, _P, _P]),
    "ddm_ilu0_nnz": (_I64, [_P]),
    "ddm_chol_host_create": (_I32, [_I64, _P, _P, _P, _I64, _P, _PP]),
    "ddm_direct_host_create": (_I32, [_I64, _P, _P, _P, _I64, _P, _I32, _PP]),
    "ddm_direct_create": (_I32, [_P, _P, _I64, _P, _I32, _D, _PP]),
    "ddm_chol_host_destroy": (None, [_P]),
    "ddm_chol_host_nnz": (_I64, [_P]),
    "ddm_chol_host_nnz_factor": (_I64, [_P]),
    "ddm_chol_host_flops": (_D, [_P]),
    "ddm_chol_host_get": (_I32, [_P, _P, _P, _P, _P]),
    "ddm_schwarz_create_ex": (_I32, [_P, _P, _I64, _P, _I64, _P, _P, _I32, ctypes.c_char_p, _P, _P, _PP]),
    "ddm_schwarz_engine": (_I32, [_P]),
    "ddm_schwarz_factor_nnz": (_I64, [_P]),
    "ddm_schwarz_status": (_I32, [_P, _P]),
    "ddm_combined_status": (_I32, [_P, _P]),
    "ddm_ilu0_get_factors_host": (_I32, [_P, _P, _P]),
    "ddm_halo_create": (_I32, [_P, _I32, _I32, _I64, _P, _P, _P, _I64, _P, _P, _P, _PP]),
    "ddm_halo_destroy": (None, [_P]),
    "ddm_halo_exchange": (_I32, [_P, _P, _P]),
    "ddm_halo_sendbuf": (_P, [_P]),
    "ddm_halo_recvbuf": (_P, [_P]),
    "ddm_op_create": (_I32, [_P, _P, _P, _P, _PP]),
    "ddm_op_destroy": (None, [_P]),
    "ddm_op_apply": (_I32, [_P, _P, _P, _P]),
    "ddm_op_applyscaleadd": (_I32, [_P, _P, _D, _P, _P]),
    "ddm_dot": (_I32, [_P, _P, _P, _P, _P]),
    "ddm_norm": (_I32, [_P, _P, _P, _P]),
    "ddm_schwarz_create": (_I32, [_P, _P, _I64, _P, _I64, _P, _P, _I32, _P, _P, _PP]),
    "ddm_schwarz_destroy": (None, [_P]),
    "ddm_schwarz_apply": (_I32, [_P, _P, _P, _P]),
    "ddm_schwarz_num_levels": (_I64, [_P, _I32]),
    "ddm_galerkin_create": (_I32, [_P, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _P, _P, _PP]),
    "ddm_galerkin_destroy": (None, [_P]),
    "ddm_galerkin_apply": (_I32, [_P, _P, _P, _P]),
    "ddm_galerkin_products": (_I32, [_P, _P, _I64, _P, _I64, _P, _I64, _I64, _P]),
    "ddm_galerkin_debug_chain": (_I32, [_P, _P, _P, _I32, _P, _P, _P, ctypes.POINTER(ctypes.c_int64)]),
    "ddm_geneo_params_default": (_I32, [ctypes.POINTER(GeneoParams)]),
    "ddm_geneo_basis": (_I32, [_P, _P, _P, _I64, _P, _P, _P, ctypes.POINTER(GeneoParams), _I64, _P, _P, _P, ctypes.POINTER(GeneoInfo)]),
    "ddm_geneo_create": (_I32, [_P, _P, _P, _I64, _P, _P, _P, ctypes.POINTER(GeneoParams), _PP]),
    "ddm_geneo_compute": (_I32, [_P, _P, _I32, _I64, _P, _P, _P, ctypes.POINTER(GeneoInfo)]),
    "ddm_geneo_refresh": (_I32, [_P, _P]),
    "ddm_geneo_state": (_I32, [_P, _P]),
    "ddm_geneo_destroy": (None, [_P]),
    "ddm_geneo_pencil_host": (_I32, [_I64, _P, _P, _P, _P, _P, _P, _P, _P, _D, _P, _P, _P, _P, _P, _P]),
    "ddm_geneo_pencil_refresh_host": (_I32, [_I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _D, _P, _P]),
    "ddm_geneo_debug_start_block": (_I32, [_P, _I64, _I32, _I32, ctypes.c_uint64, _P, _P, _P]),
    "ddm_geneo_debug_pencil": (_I32, [_P, _P, _P, _P, _P, _P, _P]),
    "ddm_msgfem_basis": (_I32, [_P, _P, _P, _I64, _P, _P, _P, _P, ctypes.POINTER(GeneoParams), _I64, _P, _P, _P, ctypes.POINTER(GeneoInfo)]),
    "ddm_svd_basis": (_I32, [_P, _P, _I64, _P, _P, _P, _P, _I32, _I32, _D, _I32, _P, _P, ctypes.POINTER(GeneoInfo)]),
    "ddm_harmonic_create": (_I32, [_P, _P, _I64, _P, _I64, _P, _I64, _P, _PP]),
    "ddm_harmonic_destroy": (None, [_P]),
    "ddm_harmonic_extend": (_I32, [_P, _P, _I32, _P, _I64]),
    "ddm_harmonic_create_classes": (_I32, [_P, _P, _I64, _P, _P, _I32, _PP]),
    "ddm_harmonic_debug_apply": (_I32, [_P, _P, _I32, _I32, _P, _I64, _P, _P, _I64]),
    "ddm_harmonic_info": (_I32, [_P, _P]),
    "ddm_harmonic_get_host": (_I32, [_P, _I32, _P, _P, _P]),
    "ddm_blockvec_gram": (_I32, [_P, _I64, _P, _P, _I64, _I32, _P, _I64, _I32, _P]),
    "ddm_blockvec_gram2_sym": (_I32, [_P, _I64, _P, _P, _I64, _P, _P, _I64, _I32, _P, _P]),
    "ddm_blockvec_rotate": (_I32, [_P, _I64, _P, _P, _I64, _I32, _P, _I32, _P, _I64, _P, _I64]),
    "ddm_csr_mm_ld": (_I32, [_P, _P, _I32, _P, _I64, _P, _I64]),
    "ddm_csr_pair_create": (_I32, [_P, _I64, _P, _P, _P, _P, _I64, _P, _PP, _PP]),
    "ddm_csr_has_row_order": (_I32, [_P]),
    "ddm_csr_mm2_ld": (_I32, [_P, _P, _P, _I32, _P, _I64, _P, _P, _I64]),
    "ddm_ilu0_solve_multi_ld": (_I32, [_P, _P, _I32, _P, _I64, _P, _I64, _I32]),
    "ddm_blockvec_rotate_multi": (_I32, [_P, _I64, _P, _I32, _P, _I64, _I32, _P, _I32, _P, _I64, _P, _I64, _I32, _I32]),
    "ddm_geneo_debug_helper": (_I32, [_P, _I32, _I64, _P, _I32, _I32, ctypes.c_uint64, _P, _I64, _P, _I64, _P, _P, _I64]),
    "ddm_dense_sym_eig_host": (_I32, [_I32, _P, _P]),
    "ddm_dense_rayleigh_ritz_host": (_I32, [_I32, _P, _P, _I32, _D, _P, _P]),
    "ddm_combined_create": (_I32, [_P, _I32, _P, _P, _P, _PP]),
    "ddm_combined_destroy": (None, [_P]),
    "ddm_combined_apply": (_I32, [_P, _P, _P, _P]),
    "ddm_cg_solve": (_I32, [_P, _P, _P, _P, _P, _D, _I32, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_gmres_solve": (_I32, [_P, _P, _P, _P, _P, _D, _I32, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_bicgstab_solve": (_I32, [_P, _P, _P, _P, _P, _D, _I32, _P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(SolveResult)]),
    "ddm_op_apply_multi": (_I32, [_P, _P, _I32, _P, _P]),
    "ddm_op_applyscaleadd_multi": (_I32, [_P, _P, _I32, _D, _P, _P]),
    "ddm_dot_multi": (_I32, [_P, _P, _I32, _P, _P, _P]),
    "ddm_schwarz_apply_multi": (_I32, [_P, _P, _I32, _P, _P]),
    "ddm_galerkin_apply_multi": (_I32, [_P, _P, _I32, _P, _P]),
    "ddm_combined_apply_multi": (_I32, [_P, _P, _I32, _P, _P]),
    "ddm_cg_solve_multi": (_I32, [_P, _P, _P, _I32, _P, _P, _D, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_cg_solve_queue": (_I32, [_P, _P, _P, _I64, _I32, _P, _P, _D, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_bicgstab_solve_queue": (_I32, [_P, _P, _P, _I64, _I32, _P, _P, _D, _I32, _P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(SolveResult)]),
    "ddm_gmres_solve_multi": (_I32, [_P, _P, _P, _I32, _P, _P, _D, _I32, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_fgmres_solve": (_I32, [_P, _P, _P, _P, _P, _D, _I32, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_fgmres_solve_multi": (_I32, [_P, _P, _P, _I32, _P, _P, _D, _I32, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_fgmres_defect_multi": (_I32, [_P, _P, _I32, _P, _P, _P, _I32, _P]),
    "ddm_fcg_solve": (_I32, [_P, _P, _P, _P, _P, _D, _I32, _I32, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_fcg_solve_multi": (_I32, [_P, _P, _P, _I32, _P, _P, _D, _I32, _I32, _I32, _P, ctypes.POINTER(SolveResult)]),
    "ddm_fcg_orth_multi": (_I32, [_P, _P, _I32, _I32, _P, _P, _P, _P, _P, _I32, _P]),
    "ddm_bcg_solve_multi": (_I32, [_P, _P, _P, _I32, _P, _P, _D, _I32, _D, _P, _P, ctypes.POINTER(SolveResult)]),
    "ddm_bcg_gram_multi": (_I32, [_P, _P, _I32, _P, _P, _P, _P]),
    "ddm_bcg_update_multi": (_I32, [_P, _P, _I32, _P, _P, _P, _P, _P, _P]),
    "ddm_bcg_direction_multi": (_I32, [_P, _P, _I32, _P, _P, _P]),
    "ddm_dense_sym_pinv_host": (_I32, [_I32, _P, _D, _P, _P]),
    "ddm_bgmres_solve_multi": (_I32, [_P, _P, _P, _I32, _P, _P, _D, _I32, _I32, _D, _P, _P, ctypes.POINTER(SolveResult)]),
    "ddm_bgmres_project_multi": (_I32, [_P, _P, _I32, _I32, _P, _P, _P]),
    "ddm_bgmres_combine_multi": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "ddm_bgmres_combine_gram_multi": (_I32, [_P, _P, _I32, _I32, _P, _P, _P, _P]),
    "ddm_dense_bgmres_factor_host": (_I32, [_I32, _P, _P, _D, _P, _P, _P]),
    "ddm_schwarz_set_multi_precision": (_I32, [_P, _I32]),
    "ddm_schwarz_set_multi_engine": (_I32, [_P, _I32]),
    "ddm_ilu0_set_multi_engine": (_I32, [_P, _P, _I32]),
    "ddm_ilu0_multi_info": (_I32, [_P, _P, _I64, _P]),
    "ddm_trsv_multi_plan_host": (_I32, [_I64, _P, _P, _I64, _P, _I32, _P, _I64, _P, _P]),
    "ddm_trsv_multi_team_host": (_I32, [_P, _I32, _I32, _I32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P]),
    "ddm_local_maps_host": (_I32, [_I64, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _I64, _P, _P]),
    "ddm_schwarz_debug_local": (_I32, [_P, _P, ctypes.POINTER(ctypes.c_int), _PP, _PP]),
    "ddm_ctx_scalars": (_P, [_P]),
    "ddm_schwarz_debug_sum_restrict": (_I32, [_P, _P, _P, _I32, _P, _P, _P, _P]),
    "ddm_debug_reduction": (_I32, [_P, _I32, _I32, _I64, _P, _P, _P, _P, _P, _I32, _P, _P, _P, _P]),
    "ddm_cg_begin": (_I32, [_P, _P, _P, _P, _P, _PP]),
    "ddm_cg_steps": (_I32, [_P, _P, _I32]),
    "ddm_cg_defect": (_I32, [_P, _P, ctypes.POINTER(ctypes.c_double)]),
    "ddm_cg_def0": (_D, [_P]),
    "ddm_cg_end": (None, [_P, _P]),
    "ddm_timing_enable": (_I32, [_P, _I32]),
    "ddm_timing_get": (_I32, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "ddm_timing_reset": (_I32, [_P]),
    "ddm_synth_q1_matrix": (_I32, [_I32, _P, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _I32]),
}

_lib = None


def load_library():
    """Loads libddm_hip.so (built by __graft_entry__.build()).  Fails loudly if it is missing."""
    global _lib
    if _lib is None:
        try:
            # torch ships its own HIP runtime: it must be in the process BEFORE libddm_hip.so is opened, so that the library binds to
            # the same libamdhip64 (the streams torch hands over belong to that runtime; with the opposite order ddm_ctx_create fails
            # with "no HIP device" on a GPU box -- seen with build() followed by smoke() in one process)
            import torch  # noqa: F401
        except ImportError:
            pass
        path = os.environ.get("DDM_HIP_LIBRARY", LIB_PATH)   # (diagnostic: an experimental build of the same sources)
        if not os.path.exists(path):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the HIP hot path)")
        L = ctypes.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)            # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Context:
    """ddm_ctx: one per process / GPU.  ``stream``: raw hipStream_t (e.g. torch's current stream)."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.ddm_ctx_create(int(device), ctypes.c_void_p(stream) if stream else None, ctypes.byref(h))
        if rc != DDM_OK:
            raise DdmError(rc, "ddm_ctx_create failed (no HIP device? the hot path has no CPU fallback)")
        self.h = h
        self._keep = []
        self.rank, self.nranks = 0, 1

    def check(self, rc):
        if rc != DDM_OK:
            raise DdmError(rc, self.lib.ddm_last_error(self.h).decode())

    def sync(self):
        self.check(self.lib.ddm_ctx_sync(self.h))

    def set_comm(self, rank, nranks, alltoall, allreduce):
        """alltoall(tag, send_ptr, recv_ptr) -> int ; allreduce(ptr, n) -> int (device pointers)."""
        a = A2A_FN(lambda user, tag, s, r: int(alltoall(tag, s, r)))
        b = ALLREDUCE_FN(lambda user, p, n: int(allreduce(p, n)))
        self._keep += [a, b]
        self.check(self.lib.ddm_ctx_set_comm(self.h, rank, nranks, a, b, None))
        self.rank, self.nranks = rank, nranks

    def rccl_unique_id(self):
        """128 bytes identifying a new RCCL communicator (call on ONE rank, distribute to all)"""
        buf = ctypes.create_string_buffer(128)
        rc = self.lib.ddm_rccl_unique_id(buf)
        if rc != DDM_OK:
            raise DdmError(rc, "ddm_rccl_unique_id failed (librccl not loadable?)")
        return buf.raw

    def set_rccl(self, rank, nranks, unique_id, self_test=False):
        """in-library exchange over RCCL / xGMI (collective over all ranks: ncclCommInitRank)"""
        assert len(unique_id) == 128
        self.check(self.lib.ddm_ctx_set_rccl(self.h, int(rank), int(nranks), ctypes.c_char_p(unique_id), int(bool(self_test))))
        self.rank, self.nranks = rank, nranks

    def comm_counts(self):
        """(all-reduces, doubles carried, grouped halo exchanges) issued so far -- as a multi-rank run launches them."""
        c = np.zeros(3, dtype=np.int64)
        self.check(self.lib.ddm_ctx_comm_counts(self.h, _hp(c)))
        return [int(v) for v in c]

    def rccl_size(self):
        """ranks of the in-library communicator as RCCL reports them (ncclCommCount); 0 = no in-library exchange"""
        c = ctypes.c_int(0)
        self.check(self.lib.ddm_ctx_rccl_size(self.h, ctypes.byref(c)))
        return c.value

    def timing(self, on=True):
        self.check(self.lib.ddm_timing_enable(self.h, int(on)))

    def timer(self, name):
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        self.check(self.lib.ddm_timing_get(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    def timing_reset(self):
        self.check(self.lib.ddm_timing_reset(self.h))

    def close(self):
        if self.h:
            self.lib.ddm_ctx_destroy(self.h)
            self.h = None


def torch_context(device=0):
    """Context bound to torch's current stream on ``device``.  If that is the legacy default stream
    (which can neither be captured into a HIP graph nor ordered against a non-blocking stream) a
    side stream is created and made current, so torch allocations / copies and the library's
    kernels are ordered on one stream."""
    import torch
    torch.cuda.set_device(device)
    s = torch.cuda.current_stream()
    if s.cuda_stream == 0:
        s = torch.cuda.Stream(device=device)
        torch.cuda.set_stream(s)
    ctx = Context(device, s.cuda_stream)
    ctx._torch_stream = s
    return ctx


def _ncols(X, Y=None):
    """columns m of an (n, m) row-major block (n-vectors count as m = 1); both blocks must have the same shape and be contiguous"""
    shape = tuple(X.shape)
    if Y is not None and tuple(Y.shape) != shape:
        raise ValueError(f"block shapes differ: {shape} and {tuple(Y.shape)}")
    for t in (X, Y):
        if t is not None and hasattr(t, "is_contiguous") and not t.is_contiguous():
            raise ValueError("block vectors must be row-major contiguous (n, m) tensors")
    return 1 if len(shape) == 1 else int(shape[1])


def _ptr(t):
    """device pointer of a torch tensor / raw int"""
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


class CsrMatrix:
    """Flattened BCRSMatrix on the device (ddm_csr)."""

    def __init__(self, ctx: Context, M, host_only=False):
        """host_only: no device copy (inputs the library only reads on the host: A_neu, B_neu of geneo_basis)"""
        import scipy.sparse as sp
        M = sp.csr_matrix(M)
        if not M.has_sorted_indices:
            M = M.sorted_indices()
        self.ctx = ctx
        self.shape = M.shape
        rp, ci, va = _np(M.indptr, np.int64), _np(M.indices, np.int32), _np(M.data, np.float64)
        h = ctypes.c_void_p()
        create = ctx.lib.ddm_csr_create_host if host_only else ctx.lib.ddm_csr_create
        ctx.check(create(ctx.h, M.shape[0], M.shape[1], _hp(rp), _hp(ci), _hp(va), ctypes.byref(h)))
        self.h = h
        self.nnz = int(M.nnz)

    def set_values(self, values):
        """new values in the matrix's pattern (nnz doubles in CSR order with sorted column indices): ddm_csr_set_values.  Objects built
        on the matrix keep the old values until their refresh() is called."""
        va = _np(values, np.float64)
        if va.shape != (self.nnz,):
            raise ValueError(f"set_values: {va.size} values for a pattern of {self.nnz} entries")
        self.ctx.check(self.ctx.lib.ddm_csr_set_values(self.ctx.h, self.h, _hp(va)))

    def mv(self, x, y):
        self.ctx.check(self.ctx.lib.ddm_csr_mv(self.ctx.h, self.h, _ptr(x), _ptr(y)))

    def usmv(self, alpha, x, y):
        self.ctx.check(self.ctx.lib.ddm_csr_usmv(self.ctx.h, self.h, float(alpha), _ptr(x), _ptr(y)))

    def mm(self, X, Y):
        """Y = A X for row-major (n, nrhs) device tensors"""
        assert X.shape == Y.shape and X.is_contiguous() and Y.is_contiguous() and X.shape[0] == self.shape[1]
        self.ctx.check(self.ctx.lib.ddm_csr_mm(self.ctx.h, self.h, int(X.shape[1]), _ptr(X), _ptr(Y)))

    def mm_ld(self, X, Y):
        """Y = A X for (n, nrhs) device tensors or column slices of wider row-major ones (ddm_csr_mm_ld, for tests)"""
        _csr_mm_ld(self.ctx, self.h, X, Y)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.lib.ddm_csr_destroy(self.h)
        except Exception:
            pass


def _block_ld(*blocks):
    """(columns, leading dimensions) of 2-d device tensors of one shape whose rows are contiguous (column slices of row-major blocks)"""
    shape = tuple(blocks[0].shape)
    for t in blocks:
        if t.dim() != 2 or tuple(t.shape) != shape or t.stride(1) != 1:
            raise ValueError("blocks must be (n, m) tensors of one shape with contiguous rows")
    return int(shape[1]), [int(t.stride(0)) for t in blocks]


def _csr_mm_ld(ctx, h, X, Y):
    m, (ldx, ldy) = _block_ld(X, Y)
    ctx.check(ctx.lib.ddm_csr_mm_ld(ctx.h, h, m, _ptr(X), ldx, _ptr(Y), ldy))


class CsrPair:
    """Two matrices on one pattern as the GenEO eigensolver makes its pencil (ddm_csr_pair_create, for tests): M gives the pattern
    and the first values, values2 (nnz, in M's sorted CSR order) the second; block_ptr: the diagonal blocks in which the cache-blocked
    row order of the block products is looked for (None: natural order)."""

    def __init__(self, ctx: Context, M, values2, block_ptr=None):
        import scipy.sparse as sp
        M = sp.csr_matrix(M)
        assert M.has_sorted_indices and M.shape[0] == M.shape[1]
        self.ctx, self.shape, self.nnz = ctx, M.shape, int(M.nnz)
        rp, ci, va, vc = _np(M.indptr, np.int64), _np(M.indices, np.int32), _np(M.data, np.float64), _np(values2, np.float64)
        assert vc.shape == va.shape
        bp = _np(block_ptr, np.int64) if block_ptr is not None else None
        self.h, self.h2 = ctypes.c_void_p(), ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_csr_pair_create(ctx.h, M.shape[0], _hp(rp), _hp(ci), _hp(va), _hp(vc), len(bp) - 1 if bp is not None else 0, _hp(bp),
                                              ctypes.byref(self.h), ctypes.byref(self.h2)))

    def has_row_order(self):
        return bool(self.ctx.lib.ddm_csr_has_row_order(self.h))

    def mm_ld(self, X, Y, second=False):
        """Y = A1 X (second: A2 X) through the single-matrix product"""
        _csr_mm_ld(self.ctx, self.h2 if second else self.h, X, Y)

    def mm2_ld(self, X, Y1, Y2):
        """Y1 = A1 X, Y2 = A2 X in one pass (ddm_csr_mm2_ld); Y1 and Y2 share their leading dimension"""
        m, (ldx, ld1, ld2) = _block_ld(X, Y1, Y2)
        assert ld1 == ld2
        self.ctx.check(self.ctx.lib.ddm_csr_mm2_ld(self.ctx.h, self.h, self.h2, m, _ptr(X), ldx, _ptr(Y1), _ptr(Y2), ld1))

    def close(self):
        if self.h and self.ctx.h:
            self.ctx.lib.ddm_csr_destroy(self.h2)
            self.ctx.lib.ddm_csr_destroy(self.h)
        self.h = self.h2 = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chol_host(M, block_ptr=None, numeric=True, general=False):
    """The host part of the sparse direct solver alone (ordering, symbolic analysis, numeric Cholesky; no device needed).
    Returns dict(perm, rowptr, col, lu, nnzL, flops); lu follows the ILU(0) storage convention over the permuted indices."""
    import scipy.sparse as sp
    lib = load_library()
    M = sp.csr_matrix(M)
    if not M.has_sorted_indices:
        M = M.sorted_indices()
    n = M.shape[0]
    bp = _np([0, n] if block_ptr is None else block_ptr, np.int64)
    rp, ci, va = _np(M.indptr, np.int64), _np(M.indices, np.int32), _np(M.data, np.float64)
    h = ctypes.c_void_p()
    rc = lib.ddm_direct_host_create(n, _hp(rp), _hp(ci), _hp(va) if numeric else None, len(bp) - 1, _hp(bp), int(general), ctypes.byref(h))
    if rc != DDM_OK:
        raise DdmError(rc, "sparse Cholesky failed (DDM_ENUMERIC: matrix not positive definite)")
    try:
        nz = lib.ddm_chol_host_nnz(h)
        out = {"perm": np.empty(n, dtype=np.int32), "rowptr": np.empty(n + 1, dtype=np.int64) if nz else None,
               "col": np.empty(nz, dtype=np.int32) if nz else None, "lu": np.empty(nz, dtype=np.float64) if nz else None,
               "nnzL": int(lib.ddm_chol_host_nnz_factor(h)), "flops": float(lib.ddm_chol_host_flops(h))}
        lib.ddm_chol_host_get(h, _hp(out["perm"]), _hp(out["rowptr"]), _hp(out["col"]), _hp(out["lu"]))
    finally:
        lib.ddm_chol_host_destroy(h)
    return out


def sn_symbolic_host(M, block_ptr=None):
    """Host half of the device supernodal Cholesky (ordering + symbolic analysis, no device needed): list of per-block dicts
    perm, first, rptr, rows, parent, level, flops, entries."""
    import scipy.sparse as sp
    lib = load_library()
    M = sp.csr_matrix(M)
    if not M.has_sorted_indices:
        M = M.sorted_indices()
    n = M.shape[0]
    bp = _np([0, n] if block_ptr is None else block_ptr, np.int64)
    rp, ci = _np(M.indptr, np.int64), _np(M.indices, np.int32)
    h = ctypes.c_void_p()
    rc = lib.ddm_sn_host_create(n, _hp(rp), _hp(ci), len(bp) - 1, _hp(bp), ctypes.byref(h))
    if rc != DDM_OK:
        raise DdmError(rc, "ddm_sn_host_create failed")
    out = []
    try:
        for b in range(len(bp) - 1):
            sz = np.zeros(4, dtype=np.int64)
            fl = ctypes.c_double()
            lib.ddm_sn_host_sizes(h, b, _hp(sz), ctypes.byref(fl))
            nsn, nrows = int(sz[0]), int(sz[1])
            d = {"perm": np.empty(int(bp[b + 1] - bp[b]), dtype=np.int32), "first": np.empty(nsn + 1, dtype=np.int32), "rptr": np.empty(nsn + 1, dtype=np.int64),
                 "rows": np.empty(nrows, dtype=np.int32), "parent": np.empty(nsn, dtype=np.int32), "level": np.empty(nsn, dtype=np.int32),
                 "flops": fl.value, "entries": int(sz[2]), "levels": int(sz[3])}
            lib.ddm_sn_host_get(h, b, _hp(d["perm"]), _hp(d["first"]), _hp(d["rptr"]), _hp(d["rows"]), _hp(d["parent"]), _hp(d["level"]))
            out.append(d)
    finally:
        lib.ddm_sn_host_destroy(h)
    return out


class Ilu0:
    """ddm_ilu0: a local factor solver -- ILU(0) in natural order, or (direct=True) the sparse Cholesky of ddm_chol_create."""

    def __init__(self, ctx: Context, A: CsrMatrix, block_ptr=None, direct=False, max_flops=0.0, general=False):
        self.ctx, self.A = ctx, A
        bp = _np([0, A.shape[0]] if block_ptr is None else block_ptr, np.int64)
        h = ctypes.c_void_p()
        if direct:
            ctx.check(ctx.lib.ddm_direct_create(ctx.h, A.h, len(bp) - 1, _hp(bp), int(general), float(max_flops), ctypes.byref(h)))
        else:
            ctx.check(ctx.lib.ddm_ilu0_create(ctx.h, A.h, len(bp) - 1, _hp(bp), ctypes.byref(h)))
        self.h = h

    @property
    def nnz(self):
        return int(self.ctx.lib.ddm_ilu0_nnz(self.h))

    def refinement(self):
        """(steps per solve, backward errors of the probe after 0, 1, .. steps) of a device direct factor."""
        om = np.zeros(5)
        steps = int(self.ctx.lib.ddm_ilu0_refinement(self.h, _hp(om)))
        return steps, om

    def sn_pivots(self):
        """the row order the pivoting of a device L U factor chose (ddm_ilu0_sn_pivots, for tests): int32[n] in the permuted
        numbering, entry first[s] + k = the block-local row of supernode s that ended in position k."""
        out = np.empty(int(self.A.shape[0]), dtype=np.int32)
        self.ctx.check(self.ctx.lib.ddm_ilu0_sn_pivots(self.ctx.h, self.h, _hp(out)))
        return out

    def refresh(self):
        """refactorises from the current values of the matrix (CsrMatrix.set_values): ddm_ilu0_refresh.  ILU(0): DdmError with code
        DDM_ENUMERIC for a vanishing pivot (the factor stays the previous one).  Device supernodal direct factor (engine()
        'supernodal'): factorised again on the kept structure, refinement decided again; its panels are overwritten, so after a
        DdmError (DDM_ENUMERIC: not positive definite; DDM_ENOTIMPL: values an unforced creation hands to the host engine) the factor
        is invalid and every solve raises DDM_ENUMERIC until a refresh succeeds.  DDM_ENOTIMPL, nothing touched, for the host-engine
        direct factor and the box engine: create a new factor."""
        self.ctx.check(self.ctx.lib.ddm_ilu0_refresh(self.ctx.h, self.h))

    def refresh_count(self):
        """successful in-place refreshes since creation (ddm_ilu0_refresh_count)"""
        return int(self.ctx.lib.ddm_ilu0_refresh_count(self.h))

    def solve(self, d, x):
        self.ctx.check(self.ctx.lib.ddm_ilu0_solve(self.ctx.h, self.h, _ptr(d), _ptr(x)))

    def solve_multi(self, D, X, single_precision=False):
        """X = (LU)^-1 D for row-major (n, nrhs) device tensors; single_precision: float sweeps (preconditioner grade)"""
        assert D.shape == X.shape and D.is_contiguous() and X.is_contiguous()
        fn = self.ctx.lib.ddm_ilu0_solve_multi_f32 if single_precision else self.ctx.lib.ddm_ilu0_solve_multi
        self.ctx.check(fn(self.ctx.h, self.h, int(D.shape[1]), _ptr(D), _ptr(X)))

    def solve_multi_ld(self, D, X, single_precision=False):
        """the same for column slices of wider row-major blocks: leading dimensions D.stride(0), X.stride(0) (ddm_ilu0_solve_multi_ld,
        for tests)"""
        m, (ldd, ldx) = _block_ld(D, X)
        self.ctx.check(self.ctx.lib.ddm_ilu0_solve_multi_ld(self.ctx.h, self.h, m, _ptr(D), ldd, _ptr(X), ldx, int(bool(single_precision))))

    def set_multi_engine(self, name):
        """engine of the block solves (ddm_ilu0_set_multi_engine): 'levels' (one launch per level, the default), 'xcd' (one persistent
        launch, same bits) or 'xcd1' (xcd with all workgroups in one team, for tests); no effect on a direct factor"""
        if name not in MULTI_ENGINES:
            raise ValueError("unknown multi engine '" + str(name) + "' (levels, xcd, xcd1)")
        self.ctx.check(self.ctx.lib.ddm_ilu0_set_multi_engine(self.ctx.h, self.h, MULTI_ENGINES.index(name)))

    def multi_info(self):
        """what the block solves run on (ddm_ilu0_multi_info, after a synchronisation): dict with `requested` and `engine` ('levels' /
        'xcd' / 'xcd1'; engine None before the first block solve), `declined` (None, 'not requested', 'direct factor', 'wide level')
        and of the last xcd launch `grid`, `teams`, `one_team`, `tickets` (workgroups per XCD)"""
        self.ctx.sync()
        out = np.zeros(14, dtype=np.int64)
        cnt = ctypes.c_int64()
        rc = self.ctx.lib.ddm_ilu0_multi_info(self.h, _hp(out), 14, ctypes.byref(cnt))
        if rc != DDM_OK or cnt.value != 14:
            raise DdmError(rc, "ddm_ilu0_multi_info failed")
        return {"requested": MULTI_ENGINES[int(out[0])], "engine": None if out[1] < 0 else MULTI_ENGINES[int(out[1])],
                "declined": (None, "not requested", "direct factor", "wide level")[int(out[2])], "grid": int(out[3]), "teams": int(out[4]),
                "one_team": bool(out[5]), "tickets": [int(v) for v in out[6:14]]}

    def num_levels(self, upper=False):
        return int(self.ctx.lib.ddm_ilu0_num_levels(self.h, int(upper)))

    def box_check(self):
        """stamps of the box engine's last solve (DDM_BOX_CHECK=1 at creation): [sweep][plane of block 0] = (start, end in 10 ns ticks,
        polls of the previous plane's progress word, XCC id)"""
        out = np.zeros(1024, dtype=np.uint64)
        self.ctx.lib.ddm_ilu0_box_check(self.h, _hp(out))
        return out.reshape(2, 128, 4)

    def box_info(self):
        """what the box engine's builder made of the matrix (ddm_ilu0_box_info, for tests): dict with `blocks` = [(nx, ny, nz, steps
        per plane, rows behind the box)], `grid` = workgroups of a sweep launch, `nested` = settled engine of the factor that solves
        the rows behind the boxes (None without such rows); no blocks for a factor that is not on the box engine"""
        cnt = ctypes.c_int64()
        rc = self.ctx.lib.ddm_ilu0_box_info(self.h, None, 0, ctypes.byref(cnt))
        out = np.zeros(cnt.value, dtype=np.int64)
        rc = rc or self.ctx.lib.ddm_ilu0_box_info(self.h, _hp(out), cnt.value, ctypes.byref(cnt))
        if rc != DDM_OK:
            raise DdmError(rc, "ddm_ilu0_box_info failed")
        return {"blocks": [tuple(int(v) for v in out[3 + 5 * b:8 + 5 * b]) for b in range(int(out[0]))], "grid": int(out[1]),
                "nested": SchwarzPreconditioner.ENGINES[int(out[2])] if out[2] >= 0 else None}

    def solve_tail(self, d, x, scale=None, add=None):
        """x = ((LU)^-1 d) * scale + add entry by entry; scale / add: device vectors or None (ddm_ilu0_solve_tail)"""
        self.ctx.check(self.ctx.lib.ddm_ilu0_solve_tail(self.ctx.h, self.h, _ptr(d), _ptr(x), _ptr(scale) if scale is not None else None,
                                                       _ptr(add) if add is not None else None))

    def wait(self):
        """joins the part of the setup that runs in the background (ddm_ilu0_wait)"""
        self.ctx.check(self.ctx.lib.ddm_ilu0_wait(self.ctx.h, self.h))

    def debug_stamps(self, d, x):
        out = np.zeros(8, dtype=np.uint64)
        self.ctx.check(self.ctx.lib.ddm_ilu0_debug_stamps(self.ctx.h, self.h, _ptr(d), _ptr(x), _hp(out)))
        return out

    def pipe_trace(self, d, x):
        """diagnostic: (stamps[ntasks, 272] uint64, meta[ntasks, 2] int32 = group, sweep) of one pipe-engine solve"""
        nt = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.ddm_ilu0_pipe_trace(self.ctx.h, self.h, None, None, None, None, 0, ctypes.byref(nt)))
        out = np.zeros((nt.value, 272), dtype=np.uint64)
        meta = np.zeros((nt.value, 2), dtype=np.int32)
        self.ctx.check(self.ctx.lib.ddm_ilu0_pipe_trace(self.ctx.h, self.h, _ptr(d), _ptr(x), _hp(out), _hp(meta), nt.value, ctypes.byref(nt)))
        return out, meta

    def pipe_info(self):
        """diagnostic: the pipe engine's queue order: a dict of the launch's workgroups, spread mode, the bound and the gap of the
        moved tasks, how many were moved per sweep and at most in one queue, and per task start level and moved flag"""
        cnt = ctypes.c_int64()
        self.ctx.check(self.ctx.lib.ddm_ilu0_pipe_info(self.ctx.h, self.h, None, 0, ctypes.byref(cnt)))
        out = np.zeros(cnt.value, dtype=np.int64)
        self.ctx.check(self.ctx.lib.ddm_ilu0_pipe_info(self.ctx.h, self.h, _hp(out), cnt.value, ctypes.byref(cnt)))
        names = ("grid", "spread", "move_max", "moved_forward", "moved_backward", "max_moved", "move_gap", "ntasks")
        info = dict(zip(names, out[:8].tolist()))
        info["start_level"], info["moved"] = out[8::2].copy(), out[9::2].copy()
        return info

    def engine(self):
        return SchwarzPreconditioner.ENGINES[int(self.ctx.lib.ddm_ilu0_engine(self.h))]

    def status(self):
        st = ctypes.c_int()
        self.ctx.check(self.ctx.lib.ddm_ilu0_status(self.ctx.h, self.h, ctypes.byref(st)))
        return st.value

    def factors(self):
        out = np.empty(self.nnz, dtype=np.float64)                # the factor's own entries: a direct factor holds its fill
        self.ctx.check(self.ctx.lib.ddm_ilu0_get_factors_host(self.ctx.h, self.h, _hp(out)))
        return out

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.lib.ddm_ilu0_destroy(self.h)
        except Exception:
            pass


class Halo:
    """One DUNE interface flattened into a pack / exchange / unpack plan (ddm_halo)."""
    COPY, ADD = 0, 1

    def __init__(self, ctx: Context, tag, mode, plan):
        self.ctx, self.tag, self.mode, self.plan = ctx, tag, mode, plan
        a = {k: _np(plan[k], np.int64) for k in ("send_idx", "send_counts", "recv_counts", "dst_idx", "dst_ptr", "src_pos")}
        assert len(a["send_counts"]) == ctx.nranks and len(a["recv_counts"]) == ctx.nranks
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_halo_create(ctx.h, tag, mode, len(a["send_idx"]), _hp(a["send_idx"]), _hp(a["send_counts"]),
                                          _hp(a["recv_counts"]), len(a["dst_idx"]), _hp(a["dst_idx"]), _hp(a["dst_ptr"]),
                                          _hp(a["src_pos"]), ctypes.byref(h)))
        self.h = h
        self.send_counts = [int(c) for c in a["send_counts"]]
        self.recv_counts = [int(c) for c in a["recv_counts"]]

    def exchange(self, v):
        self.ctx.check(self.ctx.lib.ddm_halo_exchange(self.ctx.h, self.h, _ptr(v)))

    def exchange_to(self, src, dst):
        """pack from ``src``, unpack into ``dst`` (entries outside the destination list are left alone)"""
        self.ctx.check(self.ctx.lib.ddm_halo_exchange_to(self.ctx.h, self.h, _ptr(src), _ptr(dst)))

    @property
    def sendbuf(self):
        return self.ctx.lib.ddm_halo_sendbuf(self.h)

    @property
    def recvbuf(self):
        return self.ctx.lib.ddm_halo_recvbuf(self.h)


class NonOverlappingOperator:
    """dune/ddm/nonoverlapping_operator.hh:11-58 (+ the scalar product :63-89)."""

    def __init__(self, ctx: Context, A: CsrMatrix, novlp_add: Halo | None, owner_mask):
        self.ctx, self.A, self.halo = ctx, A, novlp_add
        m = _np(owner_mask, np.uint8)
        assert len(m) == A.shape[0]
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_op_create(ctx.h, A.h, novlp_add.h if novlp_add else None, _hp(m), ctypes.byref(h)))
        self.h = h

    def refresh(self):
        """rebuilds the product's storage from the matrix's current values (CsrMatrix.set_values): ddm_op_refresh"""
        self.ctx.check(self.ctx.lib.ddm_op_refresh(self.ctx.h, self.h))

    def apply(self, x, y):
        self.ctx.check(self.ctx.lib.ddm_op_apply(self.ctx.h, self.h, _ptr(x), _ptr(y)))

    def applyscaleadd(self, alpha, x, y):
        self.ctx.check(self.ctx.lib.ddm_op_applyscaleadd(self.ctx.h, self.h, float(alpha), _ptr(x), _ptr(y)))

    def dot(self, x, y):
        r = ctypes.c_double()
        self.ctx.check(self.ctx.lib.ddm_dot(self.ctx.h, self.h, _ptr(x), _ptr(y), ctypes.byref(r)))
        return r.value

    def norm(self, x):
        r = ctypes.c_double()
        self.ctx.check(self.ctx.lib.ddm_norm(self.ctx.h, self.h, _ptr(x), ctypes.byref(r)))
        return r.value

    def apply_multi(self, X, Y):
        """Y = A X for (n, m) row-major device blocks (ddm_op_apply_multi)"""
        self.ctx.check(self.ctx.lib.ddm_op_apply_multi(self.ctx.h, self.h, _ncols(X, Y), _ptr(X), _ptr(Y)))

    def applyscaleadd_multi(self, alpha, X, Y):
        self.ctx.check(self.ctx.lib.ddm_op_applyscaleadd_multi(self.ctx.h, self.h, _ncols(X, Y), float(alpha), _ptr(X), _ptr(Y)))

    def dot_multi(self, X, Y):
        """the m owner-masked dots <X_c, Y_c> as a numpy array (ddm_dot_multi)"""
        m = _ncols(X, Y)
        r = np.zeros(max(m, 1), dtype=np.float64)
        self.ctx.check(self.ctx.lib.ddm_dot_multi(self.ctx.h, self.h, m, _ptr(X), _ptr(Y), _hp(r)))
        return r[:m]


class SchwarzPreconditioner:
    """dune/ddm/schwarz.hh:54-220 with the ILU(0) local solver on the device."""
    TYPES = {"standard": 0, "restricted": 1}

    def __init__(self, ctx: Context, A_dir: CsrMatrix, block_ptr, n_novlp, ext_map, pou, type, ovlp_copy: Halo | None,
                 ovlp_add: Halo | None, subdomain_solver="ilu0"):
        if type not in self.TYPES:
            raise NotImplementedError("Unknown Schwarz type '" + str(type) + "'")   # schwarz.hh:83
        self.ctx = ctx
        bp = _np(block_ptr, np.int64)
        em = _np(ext_map, np.int32)
        pw = None if pou is None else _np(pou, np.float64)
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_schwarz_create_ex(ctx.h, A_dir.h, len(bp) - 1, _hp(bp), int(n_novlp), _hp(em), _hp(pw), self.TYPES[type],
                                                str(subdomain_solver).encode(), ovlp_copy.h if ovlp_copy else None,
                                                ovlp_add.h if ovlp_add else None, ctypes.byref(h)))
        self.h = h
        self._keep = (A_dir, ovlp_copy, ovlp_add)

    def refresh(self):
        """the local solver again from A_dir's current values (CsrMatrix.set_values): ddm_schwarz_refresh.  ILU(0) and the device
        supernodal direct factor are refreshed in place (Ilu0.refresh says what that means for each).  DdmError with code
        DDM_ENOTIMPL for the host-engine direct factor, the box engine and a device factor whose new values belong to the host
        engine: build a new SchwarzPreconditioner instead."""
        self.ctx.check(self.ctx.lib.ddm_schwarz_refresh(self.ctx.h, self.h))

    def refresh_count(self):
        """successful in-place refreshes of the local solver since this object was created (ddm_ilu0_refresh_count)"""
        F = self.ctx.lib.ddm_schwarz_local_solver(self.h)
        return int(self.ctx.lib.ddm_ilu0_refresh_count(ctypes.c_void_p(F))) if F else 0

    def apply(self, x, d):
        self.ctx.check(self.ctx.lib.ddm_schwarz_apply(self.ctx.h, self.h, _ptr(x), _ptr(d)))

    def apply_multi(self, X, D):
        self.ctx.check(self.ctx.lib.ddm_schwarz_apply_multi(self.ctx.h, self.h, _ncols(X, D), _ptr(X), _ptr(D)))

    def set_multi_precision(self, f32):
        """f32 true: the block applies run their local solve with single-precision sweeps (ddm_schwarz_set_multi_precision; meant for
        the flexible drivers only); false (the default): double"""
        self.ctx.check(self.ctx.lib.ddm_schwarz_set_multi_precision(self.h, 1 if f32 else 0))

    def set_multi_engine(self, name):
        """engine of the local solves of the block applies (ddm_schwarz_set_multi_engine): 'levels' (the default), 'xcd' (one persistent
        launch for both sweeps of all subdomains; the same bits) or 'xcd1' (xcd with one team, for tests)"""
        if name not in MULTI_ENGINES:
            raise ValueError("unknown multi engine '" + str(name) + "' (levels, xcd, xcd1)")
        self.ctx.check(self.ctx.lib.ddm_schwarz_set_multi_engine(self.h, MULTI_ENGINES.index(name)))

    def local_solver(self):
        """the local solver object (ddm_ilu0 *, borrowed) as a raw pointer"""
        return self.ctx.lib.ddm_schwarz_local_solver(self.h)

    def num_levels(self):
        return (int(self.ctx.lib.ddm_schwarz_num_levels(self.h, 0)), int(self.ctx.lib.ddm_schwarz_num_levels(self.h, 1)))

    ENGINES = {8: "pipe", 4: "xcd2", 0: "levels", 16: "supernodal", 32: "box"}

    def engine(self):
        """triangular-solve engine of the local solver: 'box' (structured blocks: csrc/trsv_box.hpp), 'pipe', 'xcd2' (also when pipe declined
        the matrix), 'levels', or 'supernodal'
        (sparse direct factor of the device engine: dense panels, csrc/sn_chol.hpp)"""
        return self.ENGINES[int(self.ctx.lib.ddm_schwarz_engine(self.h))]

    def wait_setup(self):
        """joins the local solver's background setup (the pipe engine's schedule is built while the caller goes on, e.g. into the
        GenEO eigensolver): ddm_ilu0_wait; the first apply would wait for it otherwise"""
        F = self.ctx.lib.ddm_schwarz_local_solver(self.h)
        if F:
            self.ctx.check(self.ctx.lib.ddm_ilu0_wait(self.ctx.h, ctypes.c_void_p(F)))

    def factor_nnz(self):
        """stored entries of the local solver's factor (roofline accounting)"""
        return int(self.ctx.lib.ddm_schwarz_factor_nnz(self.h))

    def check_status(self):
        """raises DdmError if a single-launch local solve timed out since creation (synchronous)"""
        self.ctx.check(self.ctx.lib.ddm_schwarz_status(self.ctx.h, self.h))


class GalerkinPreconditioner:
    """dune/ddm/galerkin_preconditioner.hh:40-363 (apply path; the coarse matrix is assembled by
    ``coarse.build_coarse_matrix`` and handed over as its replicated inverse)."""

    def __init__(self, ctx: Context, n, n_novlp, ext_map, sub_ptr, basis, coarse_index, a0inv, ovlp_copy, ovlp_add):
        self.ctx = ctx
        basis = _np(basis, np.float64)
        kmax = basis.shape[0]
        assert basis.shape[1] == n
        sp_ = _np(sub_ptr, np.int64)
        ci = _np(coarse_index, np.int64)
        inv = _np(a0inv, np.float64)
        K = inv.shape[0]
        em = _np(ext_map, np.int32)
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_galerkin_create(ctx.h, int(n), int(n_novlp), _hp(em), len(sp_) - 1, _hp(sp_), kmax, _hp(basis), _hp(ci),
                                              K, _hp(inv), ovlp_copy.h if ovlp_copy else None, ovlp_add.h if ovlp_add else None,
                                              ctypes.byref(h)))
        self.h = h
        self.K = int(K)
        self._keep = (ovlp_copy, ovlp_add)

    def set_inverse(self, a0inv):
        """a new inverse of the coarse matrix (K x K) for the same basis: ddm_galerkin_set_inverse"""
        inv = _np(a0inv, np.float64)
        if inv.shape != (self.K, self.K):
            raise ValueError(f"set_inverse: shape {inv.shape}, the coarse space has {self.K} vectors")
        self.ctx.check(self.ctx.lib.ddm_galerkin_set_inverse(self.ctx.h, self.h, _hp(inv)))

    def apply(self, x, d):
        self.ctx.check(self.ctx.lib.ddm_galerkin_apply(self.ctx.h, self.h, _ptr(x), _ptr(d)))

    def apply_multi(self, X, D):
        self.ctx.check(self.ctx.lib.ddm_galerkin_apply_multi(self.ctx.h, self.h, _ncols(X, D), _ptr(X), _ptr(D)))

    def debug_chain(self, d_ovlp, K, spread_grid=0):
        """diagnostic: the coarse chain alone on an overlapping device defect, with the full-grid basis passes (spread_grid 0) or the
        spread ones on that many one-wave workgroups; returns device tensors (chunk partials, coarse defect, prolonged correction)"""
        import torch
        npart = ctypes.c_int64(0)
        self.ctx.check(self.ctx.lib.ddm_galerkin_debug_chain(self.ctx.h, self.h, None, int(spread_grid), None, None, None, ctypes.byref(npart)))
        partial = torch.empty(max(npart.value, 1), dtype=torch.float64, device=d_ovlp.device)
        d0 = torch.empty(max(int(K), 1), dtype=torch.float64, device=d_ovlp.device)
        xov = torch.empty_like(d_ovlp)
        self.ctx.check(self.ctx.lib.ddm_galerkin_debug_chain(self.ctx.h, self.h, _ptr(d_ovlp), int(spread_grid), _ptr(partial), _ptr(d0), _ptr(xov),
                                                             ctypes.byref(npart)))
        return partial[:npart.value], d0[:int(K)], xov


def galerkin_products(ctx: Context, A_dir: CsrMatrix, left, right, row0, row1):
    """out[i, j] = <left_i, A_dir right_j> over rows [row0, row1); left/right: torch (k x n) device tensors."""
    nl, nr = left.shape[0], right.shape[0]
    out = np.empty((nr, nl), dtype=np.float64)      # column-major nl x nr
    ctx.check(ctx.lib.ddm_galerkin_products(ctx.h, A_dir.h, nl, _ptr(left), nr, _ptr(right), int(row0), int(row1), _hp(out)))
    return out.T


class CombinedPreconditioner:
    """dune/ddm/combined_preconditioner.hh:39-180."""
    MODES = {"additive": 0, "multiplicative": 1}

    def __init__(self, ctx: Context, mode="additive", op=None, schwarz=None, galerkin=None):
        if mode not in self.MODES:
            raise NotImplementedError("Unknown apply mode in CombinedPreconditioner, use either additive or multiplicative")
        self.ctx = ctx
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_combined_create(ctx.h, self.MODES[mode], op.h if op else None, schwarz.h if schwarz else None,
                                              galerkin.h if galerkin else None, ctypes.byref(h)))
        self.h = h
        self._keep = (op, schwarz, galerkin)

    def apply(self, x, d):
        self.ctx.check(self.ctx.lib.ddm_combined_apply(self.ctx.h, self.h, _ptr(x), _ptr(d)))

    def apply_multi(self, X, D):
        self.ctx.check(self.ctx.lib.ddm_combined_apply_multi(self.ctx.h, self.h, _ncols(X, D), _ptr(X), _ptr(D)))

    def check_status(self):
        self.ctx.check(self.ctx.lib.ddm_combined_status(self.ctx.h, self.h))


def cg_solve(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, x, b, reduction=1e-10, maxit=1000,
             fixed_iterations=0, history=True):
    """dune-istl CGSolver::apply as driven by examples/poisson.cc:311-319.  x, b: device tensors;
    b is overwritten by the defect.  Returns (SolveResult, history ndarray or None)."""
    res = SolveResult()
    hist = np.zeros(max(maxit, fixed_iterations) + 1, dtype=np.float64) if history else None
    ctx.check(ctx.lib.ddm_cg_solve(ctx.h, op.h, prec.h, _ptr(x), _ptr(b), float(reduction), int(maxit), int(fixed_iterations),
                                   _hp(hist), ctypes.byref(res)))
    return res, (hist[:res.iterations + 1] if history else None)


def _solve_multi(ctx: Context, fn, op, prec, X, B, reduction, maxit, extra, history):
    """behind the *_solve_multi wrappers: the result array, the NaN-filled history, the call (extra: the driver's integer arguments after
    maxit) and the trimming of the history to the largest iteration count"""
    m = _ncols(X, B)
    res = (SolveResult * max(m, 1))()
    hist = np.full((maxit + 1, max(m, 1)), np.nan) if history else None
    ctx.check(fn(ctx.h, op.h, prec.h, m, _ptr(X), _ptr(B), float(reduction), int(maxit), *extra, _hp(hist), res))
    out = [res[c] for c in range(m)]
    if not history:
        return out, None
    iters = max([r.iterations for r in out] + [0])
    return out, hist[:iters + 1, :m]


def _gmres_solve(ctx: Context, fn, op, prec, x, b, reduction, maxit, restart, history):
    """behind gmres_solve and fgmres_solve"""
    res = SolveResult()
    hist = np.zeros(maxit + 1, dtype=np.float64) if history else None
    ctx.check(fn(ctx.h, op.h, prec.h, _ptr(x), _ptr(b), float(reduction), int(maxit), int(restart), _hp(hist), ctypes.byref(res)))
    return res, (hist[:res.iterations + 1] if history else None)


def cg_solve_multi(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, reduction=1e-10, maxit=1000, history=True):
    """m independent CGSolver::apply recurrences at once (ddm_cg_solve_multi).  X, B: (n, m) row-major device tensors (B is overwritten by
    the defects).  Returns (list of m SolveResult, history): history is (iters + 1) x m with iters the largest iteration count; the
    entries of a column after it converged are NaN (its history stops there)."""
    return _solve_multi(ctx, ctx.lib.ddm_cg_solve_multi, op, prec, X, B, reduction, maxit, (), history)


def cg_solve_queue(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, width, reduction=1e-10, maxit=1000, history=True):
    """Any number of right-hand sides through a CG block of ``width`` slots (ddm_cg_solve_queue): a slot whose column has stopped takes
    the next pending column, so the block stays full until the queue is empty.  X, B: (n, ncols) row-major device tensors; X holds the
    initial guesses and receives the solutions, B is not modified.  Returns (list of ncols SolveResult, history): history is
    (iters + 1) x ncols with iters the largest iteration count, row k of column j being that column's defect after its own k-th
    iteration (NaN after its last one)."""
    ncols = _ncols(X, B)
    res = (SolveResult * max(ncols, 1))()
    hist = np.full((maxit + 1, max(ncols, 1)), np.nan) if history and maxit >= 0 else None
    ctx.check(ctx.lib.ddm_cg_solve_queue(ctx.h, op.h, prec.h, ncols, int(width), _ptr(X), _ptr(B), float(reduction), int(maxit), _hp(hist), res))
    out = [res[c] for c in range(ncols)]
    if not history:
        return out, None
    iters = max([r.iterations for r in out] + [0])
    return out, hist[:iters + 1, :ncols]


def bicgstab_solve_queue(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, width, reduction=1e-10, maxit=1000, history=True):
    """Any number of right-hand sides through a BiCGSTAB block of ``width`` slots (ddm_bicgstab_solve_queue): every column is what
    bicgstab_solve computes on it; a slot whose column has stopped takes the next pending column at the end of the iteration.  X, B:
    (n, ncols) row-major device tensors; X holds the initial guesses and receives the solutions, B is not modified.  Returns (list of
    ncols SolveResult, history): history is (halfsteps + 1) x ncols with halfsteps the largest half-step count, row k of column j being
    that column's defect after its own k-th HALF step (NaN after its last one)."""
    ncols = _ncols(X, B)
    res = (SolveResult * max(ncols, 1))()
    nh = np.zeros(max(ncols, 1), dtype=np.int32)
    hist = np.full((2 * maxit + 1, max(ncols, 1)), np.nan) if history and maxit >= 0 else None
    ctx.check(ctx.lib.ddm_bicgstab_solve_queue(ctx.h, op.h, prec.h, ncols, int(width), _ptr(X), _ptr(B), float(reduction), int(maxit), _hp(hist),
                                               nh.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), res))
    out = [res[c] for c in range(ncols)]
    if not history:
        return out, None
    return out, hist[:max(int(nh[:ncols].max(initial=1)), 1), :ncols]


def gmres_solve_multi(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, reduction=1e-10, maxit=1000, restart=100,
                      history=True):
    """m independent RestartedGMResSolver::apply recurrences at once (ddm_gmres_solve_multi), restart cycles aligned.  X, B: (n, m)
    row-major device tensors (B is overwritten).  Returns what cg_solve_multi returns: (list of m SolveResult, (iters + 1) x m history
    whose entries after a column's last iteration are NaN)."""
    return _solve_multi(ctx, ctx.lib.ddm_gmres_solve_multi, op, prec, X, B, reduction, maxit, (int(restart),), history)


def fgmres_solve(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, x, b, reduction=1e-10, maxit=1000, restart=100,
                 history=True):
    """dune-istl RestartedFlexibleGMResSolver::apply ([solver] type = restartedflexiblegmressolver): right-preconditioned restarted
    GMRES that keeps the preconditioned directions; the history holds (estimates of) the TRUE defect norm (ddm_fgmres_solve)."""
    return _gmres_solve(ctx, ctx.lib.ddm_fgmres_solve, op, prec, x, b, reduction, maxit, restart, history)


def fgmres_solve_multi(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, reduction=1e-10, maxit=1000, restart=100,
                       history=True):
    """m independent flexible restarted GMRES recurrences at once (ddm_fgmres_solve_multi), restart cycles aligned.  Arguments and
    return value as gmres_solve_multi."""
    return _solve_multi(ctx, ctx.lib.ddm_fgmres_solve_multi, op, prec, X, B, reduction, maxit, (int(restart),), history)


def fgmres_defect_multi(ctx: Context, op: NonOverlappingOperator, active, T, B, fused=True):
    """the restart step of ddm_fgmres_solve_multi on its own: B -= T in the columns with active[c] != 0; returns the m squared
    owner-masked norms of B afterwards (ddm_fgmres_defect_multi)"""
    m = _ncols(T, B)
    act = _np(active, np.int32)
    assert act.shape == (m,)
    r = np.zeros(max(m, 1), dtype=np.float64)
    ctx.check(ctx.lib.ddm_fgmres_defect_multi(ctx.h, op.h, m, _hp(act), _ptr(T), _ptr(B), 1 if fused else 0, _hp(r)))
    return r[:m]


def fcg_solve(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, x, b, reduction=1e-10, maxit=1000, mmax=10, complete=False,
              history=True):
    """dune-istl RestartedFCGSolver::apply ([solver] type = restartedfcgsolver) or, with complete=True, CompleteFCGSolver::apply
    (completefcgsolver): flexible CG for a symmetric positive definite operator with a preconditioner that is not symmetric or not
    fixed; mmax + 1 slots of stored directions; the history holds the TRUE defect norm (ddm_fcg_solve)."""
    res = SolveResult()
    hist = np.zeros(maxit + 1, dtype=np.float64) if history else None
    ctx.check(ctx.lib.ddm_fcg_solve(ctx.h, op.h, prec.h, _ptr(x), _ptr(b), float(reduction), int(maxit), int(mmax), 1 if complete else 0, _hp(hist),
                                    ctypes.byref(res)))
    return res, (hist[:res.iterations + 1] if history else None)


def fcg_solve_multi(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, reduction=1e-10, maxit=1000, mmax=10, complete=False,
                    history=True):
    """m independent flexible CG recurrences at once (ddm_fcg_solve_multi); all columns share the slot index.  Arguments and return
    value as gmres_solve_multi."""
    return _solve_multi(ctx, ctx.lib.ddm_fcg_solve_multi, op, prec, X, B, reduction, maxit, (int(mmax), 1 if complete else 0), history)


def fcg_orth_multi(ctx: Context, op: NonOverlappingOperator, active, AD, DS, g, W, fused=True):
    """one orthogonalisation of ddm_fcg_solve_multi on its own: W (n x m, device, overwritten in the columns with active[c] != 0) against
    the nslots stored blocks DS / AD (nslots x n x m device tensors, or None with nslots = 0), g: nslots x m host array of <d_k, Ad_k>;
    returns the nslots x m coefficients <Ad_k, W> / g_k (ddm_fcg_orth_multi)"""
    m = _ncols(W, W)
    act = _np(active, np.int32)
    gh = np.ascontiguousarray(np.asarray(g, dtype=np.float64).reshape(-1, m))
    nslots = gh.shape[0]
    assert act.shape == (m,) and (nslots == 0 or (tuple(AD.shape) == tuple(DS.shape) == (nslots,) + tuple(W.shape)))
    coef = np.zeros((max(nslots, 1), m), dtype=np.float64)
    ctx.check(ctx.lib.ddm_fcg_orth_multi(ctx.h, op.h, m, nslots, _hp(act), _ptr(AD) if nslots else None, _ptr(DS) if nslots else None,
                                         _hp(gh) if nslots else None, _ptr(W), 1 if fused else 0, _hp(coef)))
    return coef[:nslots]


# Default rank_tol of block CG (DDM_BCG_RANK_TOL_DEFAULT of include/ddm_hip.h): the relative eigenvalue of the Jacobi-scaled coupling
# matrix P^T A P below which a direction counts as dependent.  Chosen on the numpy restatement (tests/bcg_reference.py) with the degenerate
# block of tests/test_bcg_cpu.py (b, random, 2 b, zero, random; golden 12^3 problem, reduction 1e-10) by the gap between the recomputed true
# reduction and the reported one: every value from 1e-15 to 1e-6 gives the same run (rank 3 in every iteration, iterations 30, 28, 30, 0,
# 28, gap 4.5e-18); 1e-16 lets rounding noise through as a fourth direction in some iterations, which costs iterations (35, 30, 35, 0, 30;
# gap 7.7e-17, still converging).  1e-12, the value the algorithm was first run with, sits three decades above the lower edge of that
# plateau and is confirmed (tests/test_bcg_cpu.py::test_rank_tol_default prints the table).
BCG_RANK_TOL = 1e-12


def bcg_solve_multi(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, reduction=1e-10, maxit=1000, rank_tol=BCG_RANK_TOL,
                    history=True):
    """Block CG (ddm_bcg_solve_multi): the m columns share ONE search space; operator and preconditioner symmetric positive definite.
    X, B: (n, m) row-major device tensors (B is overwritten by the defects).  Returns (list of m SolveResult, history, ranks): history
    is (k_end + 1) x m, every row written for every column (no column is frozen); ranks[k - 1] = rank of the coupling matrix in
    iteration k = 1 .. k_end.  res[c].iterations = the first iteration at which column c passed its test."""
    m = _ncols(X, B)
    res = (SolveResult * max(m, 1))()
    hist = np.full((maxit + 1, max(m, 1)), np.nan) if maxit >= 0 else None
    ranks = np.zeros(max(maxit, 0) + 1, dtype=np.int32)
    ctx.check(ctx.lib.ddm_bcg_solve_multi(ctx.h, op.h, prec.h, m, _ptr(X), _ptr(B), float(reduction), int(maxit), float(rank_tol), _hp(hist), _hp(ranks), res))
    out = [res[c] for c in range(m)]
    k_end = int(np.sum(~np.isnan(hist[:, 0]))) - 1
    return out, (hist[:k_end + 1, :m] if history else None), ranks[1:k_end + 1].copy()


def bcg_gram_multi(ctx: Context, op: NonOverlappingOperator, U, V1, V2=None):
    """the Gram pass of block CG on its own: returns U^T V1 (m x m) or, with V2, the pair (U^T V1, U^T V2); owner-masked, summed over
    the ranks (ddm_bcg_gram_multi)"""
    m = _ncols(U, V1)
    if V2 is not None:
        _ncols(U, V2)
    G = np.full((2 if V2 is not None else 1, m, m), np.nan)       # (every entry must be written)
    ctx.check(ctx.lib.ddm_bcg_gram_multi(ctx.h, op.h, m, _ptr(U), _ptr(V1), _ptr(V2) if V2 is not None else None, _hp(G)))
    return (G[0], G[1]) if V2 is not None else G[0]


def bcg_update_multi(ctx: Context, op: NonOverlappingOperator, alpha, P, Q, X, R):
    """the update pass of block CG on its own: X += P alpha, R -= Q alpha (alpha: m x m host array); returns the m squared owner-masked
    norms of R afterwards (ddm_bcg_update_multi)"""
    m = _ncols(P, Q)
    _ncols(X, R)
    _ncols(P, X)
    a = _np(alpha, np.float64)
    assert a.shape == (m, m)
    r = np.full(m, np.nan)
    ctx.check(ctx.lib.ddm_bcg_update_multi(ctx.h, op.h, m, _hp(a), _ptr(P), _ptr(Q), _ptr(X), _ptr(R), _hp(r)))
    return r


def bcg_direction_multi(ctx: Context, op: NonOverlappingOperator, beta, Z, P):
    """the direction pass of block CG on its own: P = Z + P beta in place (beta: m x m host array; ddm_bcg_direction_multi)"""
    m = _ncols(Z, P)
    b = _np(beta, np.float64)
    assert b.shape == (m, m)
    ctx.check(ctx.lib.ddm_bcg_direction_multi(ctx.h, op.h, m, _hp(b), _ptr(Z), _ptr(P)))
    ctx.sync()


def dense_sym_pinv_host(W, tol=BCG_RANK_TOL):
    """pseudo-inverse of the symmetrised m x m matrix W as block CG forms it on the host (ddm_dense_sym_pinv_host; no device needed):
    returns (Wpinv, rank)"""
    Wc = _np(W, np.float64)
    m = Wc.shape[0]
    assert Wc.shape == (m, m)
    out = np.zeros((m, m), dtype=np.float64)
    rank = ctypes.c_int(0)
    rc = load_library().ddm_dense_sym_pinv_host(m, _hp(Wc), float(tol), _hp(out), ctypes.byref(rank))
    if rc != 0:
        raise DdmError(rc, load_library().ddm_last_error(None).decode())
    return out, int(rank.value)


# Default rank_tol of block GMRES (DDM_BGMRES_RANK_TOL_DEFAULT of include/ddm_hip.h): the relative eigenvalue of the scaled Gram matrix of
# a block below which a direction counts as dependent.  Confirmed on the numpy restatement (tests/bgmres_reference.py) with the
# degenerate block of tests/test_bgmres_cpu.py by the gap between the recomputed and the monitored reduction:
# tests/test_bgmres_cpu.py::test_rank_tol_default prints the table and states the plateau.
BGMRES_RANK_TOL = 1e-12


def bgmres_solve_multi(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, X, B, reduction=1e-10, maxit=1000, restart=100,
                       rank_tol=BGMRES_RANK_TOL, history=True):
    """Block GMRES (ddm_bgmres_solve_multi): the m columns share ONE Krylov space; right preconditioning with a fixed preconditioner,
    which need not be symmetric.  X, B: (n, m) row-major device tensors (B is overwritten by the defects).  maxit counts block
    iterations.  Returns (list of m SolveResult, history, widths): history is (k_end + 1) x m, the monitored defects, recomputed at
    every cycle end; widths[k - 1] = width of the cycle that block iteration k = 1 .. k_end belongs to.  res[c].iterations = the first
    block iteration at which column c passed its test and stayed passed."""
    m = _ncols(X, B)
    res = (SolveResult * max(m, 1))()
    hist = np.full((maxit + 1, max(m, 1)), np.nan) if maxit >= 0 else None
    widths = np.zeros(max(maxit, 0) + 1, dtype=np.int32)
    ctx.check(ctx.lib.ddm_bgmres_solve_multi(ctx.h, op.h, prec.h, m, _ptr(X), _ptr(B), float(reduction), int(maxit), int(restart), float(rank_tol),
                                             _hp(hist), _hp(widths), res))
    out = [res[c] for c in range(m)]
    k_end = int(np.sum(~np.isnan(hist[:, 0]))) - 1
    return out, (hist[:k_end + 1, :m] if history else None), widths[1:k_end + 1].copy()


def bgmres_project_multi(ctx: Context, op: NonOverlappingOperator, V, W):
    """the projection pass of block GMRES on its own: V a (K, n, p) device tensor of K stored blocks, W (n, p); returns the K matrices
    V_k^T W as a (K, p, p) array, owner-masked, summed over the ranks (ddm_bgmres_project_multi)"""
    K, p = int(V.shape[0]), _ncols(W)
    assert tuple(V.shape[1:]) == tuple(W.shape) and V.is_contiguous()
    H = np.full((K, p, p), np.nan)                                 # (every entry must be written)
    ctx.check(ctx.lib.ddm_bgmres_project_multi(ctx.h, op.h, p, K, _ptr(V), _ptr(W), _hp(H)))
    return H


def bgmres_combine_multi(ctx: Context, op: NonOverlappingOperator, mode, V, coef, Out):
    """the combination pass of block GMRES on its own: Out (n, q) = (mode 0) / += (1) / -= (2) sum_k V[k] coef[k], V a (K, n, pin)
    device tensor, coef a (K, pin, q) host array (ddm_bgmres_combine_multi)"""
    K, pin, q = int(V.shape[0]), int(V.shape[2]), _ncols(Out)
    c = _np(coef, np.float64)
    assert c.shape == (K, pin, q) and V.is_contiguous() and int(V.shape[1]) == int(Out.shape[0])
    ctx.check(ctx.lib.ddm_bgmres_combine_multi(ctx.h, op.h, int(mode), pin, q, K, _ptr(V), _hp(c), _ptr(Out)))
    ctx.sync()


def bgmres_combine_gram_multi(ctx: Context, op: NonOverlappingOperator, V, coef, W):
    """W (n, p) -= sum_k V[k] coef[k] and, from the same pass, W^T W afterwards as a (p, p) array, owner-masked, summed over the ranks
    (ddm_bgmres_combine_gram_multi)"""
    K, p = int(V.shape[0]), _ncols(W)
    c = _np(coef, np.float64)
    assert c.shape == (K, p, p) and tuple(V.shape[1:]) == tuple(W.shape) and V.is_contiguous()
    G = np.full((p, p), np.nan)
    ctx.check(ctx.lib.ddm_bgmres_combine_gram_multi(ctx.h, op.h, p, K, _ptr(V), _hp(c), _ptr(W), _hp(G)))
    return G


def dense_bgmres_factor_host(G, scale2=None, tol=BGMRES_RANK_TOL):
    """the factor of the p x p Gram matrix of a block as block GMRES forms it on the host (ddm_dense_bgmres_factor_host; no device
    needed): returns (S (rank, p) with S^T S = G, C (p, rank) with C^T G C = I, rank)"""
    Gc = _np(G, np.float64)
    p = Gc.shape[0]
    assert Gc.shape == (p, p)
    sc = _np(scale2, np.float64) if scale2 is not None else None
    assert sc is None or sc.shape == (p,)
    S = np.zeros((p, p), dtype=np.float64)
    C = np.zeros((p, p), dtype=np.float64)
    rank = ctypes.c_int(0)
    rc = load_library().ddm_dense_bgmres_factor_host(p, _hp(Gc), _hp(sc), float(tol), _hp(S), _hp(C), ctypes.byref(rank))
    if rc != 0:
        raise DdmError(rc, load_library().ddm_last_error(None).decode())
    r = int(rank.value)
    return S[:r].copy(), C[:, :r].copy(), r


def gmres_solve(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, x, b, reduction=1e-10, maxit=1000, restart=100,
                history=True):
    """dune-istl RestartedGMResSolver::apply ([solver] type = restartedgmressolver, examples/poisson.ini:12-17)."""
    return _gmres_solve(ctx, ctx.lib.ddm_gmres_solve, op, prec, x, b, reduction, maxit, restart, history)


def bicgstab_solve(ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, x, b, reduction=1e-10, maxit=1000, history=True):
    """dune-istl BiCGSTABSolver::apply ([solver] type = bicgstabsolver); history: one entry per HALF step"""
    res = SolveResult()
    hist = np.zeros(2 * maxit + 2, dtype=np.float64)
    nh = ctypes.c_int32(0)
    ctx.check(ctx.lib.ddm_bicgstab_solve(ctx.h, op.h, prec.h, _ptr(x), _ptr(b), float(reduction), int(maxit), _hp(hist), ctypes.byref(nh), ctypes.byref(res)))
    return res, (hist[:nh.value] if history else None)


class CgIteration:
    """ddm_cg_begin / steps / defect / end: the CG loop in pieces (exact-K timing in bench.py)."""

    def __init__(self, ctx: Context, op: NonOverlappingOperator, prec: CombinedPreconditioner, x, b):
        self.ctx = ctx
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_cg_begin(ctx.h, op.h, prec.h, _ptr(x), _ptr(b), ctypes.byref(h)))
        self.h = h
        self._keep = (op, prec, x, b)
        self.def0 = ctx.lib.ddm_cg_def0(h)

    def steps(self, k):
        self.ctx.check(self.ctx.lib.ddm_cg_steps(self.ctx.h, self.h, int(k)))

    def defect(self):
        d = ctypes.c_double()
        self.ctx.check(self.ctx.lib.ddm_cg_defect(self.ctx.h, self.h, ctypes.byref(d)))
        return d.value

    def end(self):
        if self.h:
            self.ctx.lib.ddm_cg_end(self.ctx.h, self.h)
            self.h = None


class HarmonicExtension:
    """ddm_harmonic: EnergyMinimalExtension (dune/ddm/coarsespaces/energy_minimal_extension.hh:36-229) on the device."""

    def __init__(self, ctx: Context, A: "CsrMatrix", interior, boundary, block_ptr=None):
        self.ctx = ctx
        ii, bb = _np(interior, np.int64), _np(boundary, np.int64)
        bp = _np(block_ptr if block_ptr is not None else [0, A.shape[0]], np.int64)
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_harmonic_create(ctx.h, A.h, len(bp) - 1, _hp(bp), len(ii), _hp(ii), len(bb), _hp(bb), ctypes.byref(h)))
        self.h = h

    @classmethod
    def from_classes(cls, ctx: Context, A: "CsrMatrix", classes, block_ptr=None, transpose=True):
        """ddm_harmonic_create_classes: classes[n] = 0 interior, 1 boundary, anything else neither; transpose: with G_bi (tests)"""
        self = cls.__new__(cls)
        self.ctx, self.h = ctx, None
        c = _np(classes, np.uint8)
        assert c.shape == (A.shape[0],)
        bp = _np(block_ptr if block_ptr is not None else [0, A.shape[0]], np.int64)
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.ddm_harmonic_create_classes(ctx.h, A.h, len(bp) - 1, _hp(bp), _hp(c), int(bool(transpose)), ctypes.byref(h)))
        self.h = h
        return self

    def debug_apply(self, op, X, pou_int=None, Y=None):
        """ddm_harmonic_debug_apply on row-major device views (n, nrhs) with any row stride: op 0 extension, 1 P, 2 P^T (in place),
        3 Y = T T^T X with the host vector pou_int (tests)"""
        assert X.dim() == 2 and X.stride(1) == 1 and (Y is None or (Y.shape == X.shape and Y.stride(1) == 1))
        d = _np(pou_int, np.float64) if pou_int is not None else None
        self.ctx.check(self.ctx.lib.ddm_harmonic_debug_apply(self.ctx.h, self.h, int(op), X.shape[1], _ptr(X), X.stride(0), _hp(d),
                                                             _ptr(Y) if Y is not None else None, Y.stride(0) if Y is not None else 0))

    def info(self):
        """ddm_harmonic_info as a dict (tests)"""
        o = np.zeros(8, dtype=np.int64)
        assert self.ctx.lib.ddm_harmonic_info(self.h, _hp(o)) == DDM_OK
        keys = ("n", "symmetric", "nnz_gib", "nnz_gbi", "supernodal", "factor_nnz", "refine_steps", "work_cols")
        return {k: int(v) for k, v in zip(keys, o)}

    def host_matrix(self, which):
        """G_ib (which = 0) or G_bi (1) as the library holds it: (rowptr, col, val) (tests)"""
        i = self.info()
        nnz = i["nnz_gbi"] if which else i["nnz_gib"]
        if nnz < 0:
            raise ValueError("the object has no G_bi")
        rp, ci, va = np.empty(i["n"] + 1, dtype=np.int64), np.empty(nnz, dtype=np.int32), np.empty(nnz, dtype=np.float64)
        assert self.ctx.lib.ddm_harmonic_get_host(self.h, int(which), _hp(rp), _hp(ci), _hp(va)) == DDM_OK
        return rp, ci, va

    def extend(self, X):
        """in place on a row-major device tensor (n, nrhs) holding the boundary values: interior rows are overwritten"""
        assert X.dim() == 2 and X.stride(1) == 1
        self.ctx.check(self.ctx.lib.ddm_harmonic_extend(self.ctx.h, self.h, X.shape[1], _ptr(X), X.stride(0)))
        return X

    def close(self):
        if self.h:
            self.ctx.lib.ddm_harmonic_destroy(self.h)
            self.h = None

    __del__ = close


def row_order_tiled_host(block_ptr, A):
    """(found, order): the cache-blocked row order of the block products for a scipy CSR matrix (host only, no device needed)"""
    lib = load_library()
    bp = _np(block_ptr, np.int64)
    rp = _np(A.indptr, np.int64)
    ci = _np(A.indices, np.int32)
    order = np.empty(A.shape[0], dtype=np.int32)
    rc = lib.ddm_csr_row_order_tiled_host(len(bp) - 1, _hp(bp), _hp(rp), _hp(ci), _hp(order))
    if rc < 0:
        raise ValueError("ddm_csr_row_order_tiled_host: bad arguments")
    return bool(rc), order


def dia_build_and_apply_host(A, x):
    """(y, blocks, counts): the operator's diagonal-row-block layout of a square scipy CSR matrix (sorted indices), applied to x on
    the host as the device kernel indexes it.  blocks: (nblocks, 4) array of (first row, end row, diagonals; 0 = CSR-stream block,
    slabs stored: fewer than the diagonals in a symmetric segment); counts: dict(blocks, dia, csr, rows_dia, slots, segments,
    symmetric_segments).  Host only, no device needed."""
    lib = load_library()
    n = A.shape[0]
    rp, ci, va = _np(A.indptr, np.int64), _np(A.indices, np.int32), _np(A.data, np.float64)
    x = _np(x, np.float64)
    y = np.full(n, np.nan)
    kinds = np.zeros((n + 1, 4), dtype=np.int32)
    counts = np.zeros(7, dtype=np.int64)
    rc = lib.ddm_dia_build_and_apply_host(n, _hp(rp), _hp(ci), _hp(va), _hp(x), _hp(y), n + 1, _hp(kinds), _hp(counts))
    if rc != DDM_OK:
        raise ValueError("ddm_dia_build_and_apply_host: bad arguments")
    return y, kinds[:counts[0]], dict(zip(("blocks", "dia", "csr", "rows_dia", "slots", "segments", "symmetric_segments"), counts.tolist()))


def trsv_multi_plan_host(A, block_ptr, upper):
    """(off, blk_nlev): the plan of the single-launch block solve for one triangle of the pattern of A (ddm_trsv_multi_plan_host) --
    off[l, b] = first position of diagonal block b among the rows of level l (off[l, nblocks] = rows of the level), blk_nlev[b] = levels
    of block b.  Host only."""
    lib = load_library()
    n = A.shape[0]
    rp, ci, bp = _np(A.indptr, np.int64), _np(A.indices, np.int32), _np(block_ptr, np.int64)
    nb = len(bp) - 1
    nlev = ctypes.c_int64()
    rc = lib.ddm_trsv_multi_plan_host(n, _hp(rp), _hp(ci), nb, _hp(bp), int(bool(upper)), None, 0, None, ctypes.byref(nlev))
    off = np.zeros((max(nlev.value, 1), nb + 1), dtype=np.int32)
    bn = np.zeros(nb, dtype=np.int32)
    rc = rc or lib.ddm_trsv_multi_plan_host(n, _hp(rp), _hp(ci), nb, _hp(bp), int(bool(upper)), _hp(off), off.size, _hp(bn), ctypes.byref(nlev))
    if rc != DDM_OK:
        raise ValueError("ddm_trsv_multi_plan_host: bad arguments")
    return off[:nlev.value], bn


def trsv_multi_team_host(tickets, nblocks, xcc, xcd_ticket, global_ticket, force_one=False):
    """dict(teams, team, rank, size, one_team) of one workgroup of the single-launch block solve (ddm_trsv_multi_team_host); tickets:
    workgroups per XCD (8 values), the grid is their sum.  Host only."""
    lib = load_library()
    tk = _np(tickets, np.uint32)
    assert len(tk) == 8
    out = np.zeros(5, dtype=np.int32)
    rc = lib.ddm_trsv_multi_team_host(_hp(tk), int(nblocks), int(bool(force_one)), int(xcc), int(xcd_ticket), int(global_ticket), int(tk.sum()), _hp(out))
    if rc != DDM_OK:
        raise ValueError("ddm_trsv_multi_team_host: bad arguments")
    return dict(teams=int(out[0]), team=int(out[1]), rank=int(out[2]), size=int(out[3]), one_team=bool(out[4]))


def local_maps_host(n, n_novlp, ext_map, plan_copy, plan_add):
    """dict(src_of, own_of, cp_ptr, cp_idx) or None: the index tables of the rank-local Schwarz passes (ddm_local_maps_host) for an
    extension map and the copy / add plans as Halo takes them (None: no exchange).  None where the tables do not exist.  Host only."""
    lib = load_library()
    em = _np(ext_map, np.int32)
    assert len(em) == n
    args, keep, max_cp = [], [], 0
    for plan in (plan_copy, plan_add):
        if plan is None:
            args += [0, None, 0, None, None, None]
            continue
        a = {k: _np(plan[k], np.int64) for k in ("send_idx", "dst_idx", "dst_ptr", "src_pos")}
        keep.append(a)
        max_cp = len(a["src_pos"])
        args += [len(a["send_idx"]), _hp(a["send_idx"]), len(a["dst_idx"]), _hp(a["dst_idx"]), _hp(a["dst_ptr"]), _hp(a["src_pos"])]
    src_of, own_of = np.empty(max(n, 1), dtype=np.int32), np.empty(max(n_novlp, 1), dtype=np.int32)
    cp_ptr, cp_idx = np.empty(n_novlp + 1, dtype=np.int32), np.empty(max(max_cp, 1), dtype=np.int32)
    counts = np.zeros(2, dtype=np.int64)
    rc = lib.ddm_local_maps_host(int(n), int(n_novlp), _hp(em), *args, _hp(src_of), _hp(own_of), _hp(cp_ptr), max_cp, _hp(cp_idx), _hp(counts))
    if rc != DDM_OK:
        raise ValueError("ddm_local_maps_host: bad arguments")
    if not counts[0]:
        return None
    return dict(src_of=src_of[:n], own_of=own_of[:n_novlp], cp_ptr=cp_ptr, cp_idx=cp_idx[:counts[1]])


def dia_windows_host(A):
    """(segments, capacity): the x windows of the same layout.  segments: one dict(staged, window, runs) per segment, runs a list of
    (first offset, doubles, window position); capacity: the doubles the windows of a staged segment may take.  Host only."""
    lib = load_library()
    n = A.shape[0]
    rp, ci, va = _np(A.indptr, np.int64), _np(A.indices, np.int32), _np(A.data, np.float64)
    max_segs, max_runs = n + 1, 32 * (n + 1)
    segs = np.zeros((max_segs, 4), dtype=np.int32)
    runs = np.zeros((max_runs, 3), dtype=np.int32)
    counts = np.zeros(4, dtype=np.int64)
    rc = lib.ddm_dia_windows_host(n, _hp(rp), _hp(ci), _hp(va), max_segs, _hp(segs), max_runs, _hp(runs), _hp(counts))
    if rc != DDM_OK:
        raise ValueError("ddm_dia_windows_host: bad arguments")
    out = [dict(staged=bool(s[0]), window=int(s[2]), runs=[tuple(r) for r in runs[s[3]:s[3] + s[1]].tolist()]) for s in segs[:counts[0]]]
    return out, int(counts[2])


def dia_codes_host(A, threads=0, arrays=True):
    """dict(coded, entries, slabs, dictionaries, codes, slots_built): the coded blocks of the same layout.  Per block: whether a
    dictionary of at most 16 values and 4-bit codes stand for its values, the dictionary entries in use (0: not coded) and whether
    its segment has value slabs; dictionaries: (coded blocks, 16) doubles in block order; codes: (rows, 4) uint32 words, nibble k
    for diagonal k (both None with arrays=False); slots_built: doubles of the slabs that were built.  `threads`: host workers
    of the build (0: the library's own number).  Host only."""
    lib = load_library()
    n = A.shape[0]
    rp, ci, va = _np(A.indptr, np.int64), _np(A.indices, np.int32), _np(A.data, np.float64)
    blocks = np.zeros((n + 1, 3), dtype=np.int32)
    dicts = np.zeros((n + 1, 16), dtype=np.float64) if arrays else None
    codes = np.zeros((n, 4), dtype=np.uint32) if arrays else None
    counts = np.zeros(5, dtype=np.int64)
    rc = lib.ddm_dia_codes_host(n, _hp(rp), _hp(ci), _hp(va), int(threads), n + 1, _hp(blocks), _hp(dicts), _hp(codes), _hp(counts))
    if rc != DDM_OK:
        raise ValueError("ddm_dia_codes_host: bad arguments")
    assert counts[3] == 16 and counts[4] == 4
    blocks = blocks[:counts[0]]
    return dict(coded=blocks[:, 0] >= 0, entries=blocks[:, 1].copy(), slabs=blocks[:, 2].astype(bool),
                dictionaries=dicts[:counts[1]] if arrays else None, codes=codes, slots_built=int(counts[2]))


def blockvec_gram(ctx: Context, sub_ptr, U, V):
    """per-subdomain U^T V of device tensors (n, pu), (n, pv) with contiguous rows (column slices of row-major blocks: the leading
    dimensions are their row strides; U and V may be the same tensor) -> ndarray (nsub, pu, pv)"""
    bp = _np(sub_ptr, np.int64)
    assert U.dim() == V.dim() == 2 and U.stride(1) == V.stride(1) == 1 and U.shape[0] == V.shape[0] == bp[-1]
    out = np.empty((len(bp) - 1, U.shape[1], V.shape[1]), dtype=np.float64)
    ctx.check(ctx.lib.ddm_blockvec_gram(ctx.h, len(bp) - 1, _hp(bp), _ptr(U), U.stride(0), U.shape[1], _ptr(V), V.stride(0), V.shape[1], _hp(out)))
    return out


def blockvec_gram2_sym(ctx: Context, sub_ptr, U, V1, V2):
    """per-subdomain U^T V1, U^T V2 for symmetric products (upper tiles computed, mirrored) -> two ndarrays (nsub, p, p)"""
    bp = _np(sub_ptr, np.int64)
    p = U.shape[1]
    assert V1.shape == U.shape == V2.shape and V1.stride(0) == V2.stride(0) and U.shape[0] == bp[-1]
    g1 = np.empty((len(bp) - 1, p, p), dtype=np.float64)
    g2 = np.empty_like(g1)
    ctx.check(ctx.lib.ddm_blockvec_gram2_sym(ctx.h, len(bp) - 1, _hp(bp), _ptr(U), U.stride(0), _ptr(V1), _ptr(V2), V1.stride(0), p, _hp(g1), _hp(g2)))
    return g1, g2


def blockvec_rotate(ctx: Context, sub_ptr, U, Y, out, base=None):
    """out[rows of s] = (base[rows of s] -) U[rows of s] @ Y[s]; U (n, p), Y ndarray (nsub, p, q), out (n, >= q) device tensors"""
    bp = _np(sub_ptr, np.int64)
    Yh = _np(Y, np.float64)
    ctx.check(ctx.lib.ddm_blockvec_rotate(ctx.h, len(bp) - 1, _hp(bp), _ptr(U), U.stride(0), U.shape[1], _hp(Yh), Yh.shape[2],
                                          _ptr(base) if base is not None else None, base.stride(0) if base is not None else 0, _ptr(out), out.stride(0)))


def blockvec_rotate_multi(ctx: Context, sub_ptr, U, Y, out, base=None, gap_from=1 << 30, gap=0):
    """out[k][rows of s, c(j)] = (base[k][rows of s, j] -) U[k][rows of s] @ Y[s][:, j] for up to three arrays that share Y (lists of
    device tensors with contiguous rows and one row stride per list); c(j) = j for j < gap_from, j + gap from there on: the rotation
    as the eigensolver's Rayleigh-Ritz step and its orthogonalisation run it (ddm_blockvec_rotate_multi, for tests)"""
    bp = _np(sub_ptr, np.int64)
    Yh = _np(Y, np.float64)
    narr, p, q = len(U), int(Yh.shape[1]), int(Yh.shape[2])
    assert 1 <= narr <= 3 and len(out) == narr and (base is None or len(base) == narr) and Yh.shape[0] == len(bp) - 1
    lds = []
    for group in (U, out, base):
        if group is None:
            lds.append(0)
            continue
        assert all(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) == group[0].stride(0) and t.shape[0] == bp[-1] for t in group)
        lds.append(int(group[0].stride(0)))
    assert all(t.shape[1] >= p for t in U)
    arr = ctypes.c_void_p * narr
    pu, po = arr(*[t.data_ptr() for t in U]), arr(*[t.data_ptr() for t in out])
    pb = arr(*[t.data_ptr() for t in base]) if base is not None else None
    ctx.check(ctx.lib.ddm_blockvec_rotate_multi(ctx.h, len(bp) - 1, _hp(bp), narr, pu, lds[0], p, _hp(Yh), q, pb, lds[2], po, lds[1], int(gap_from), int(gap)))


def _geneo_helper(ctx, op, sub_ptr, m, out, ldo, a=None, lda=0, b=None, ldb=0, s=None, nev=0, seed=0):
    bp = _np(sub_ptr, np.int64)
    ctx.check(ctx.lib.ddm_geneo_debug_helper(ctx.h, op, len(bp) - 1, _hp(bp), int(m), int(nev), int(seed), _ptr(a) if a is not None else None, int(lda),
                                             _ptr(b) if b is not None else None, int(ldb), _ptr(s) if s is not None else None, _ptr(out), int(ldo)))


def geneo_random(ctx: Context, sub_ptr, seed, mask, X):
    """k_geneo_random as the eigensolver launches it: X[i, j] = uniform[-0.5, 0.5)(seed, i m + j) * mask[i] into the (n, m) view X"""
    m, (ld,) = _block_ld(X)
    _geneo_helper(ctx, 0, sub_ptr, m, X, ld, a=mask, seed=seed)


def geneo_residual(ctx: Context, sub_ptr, mu, AX, CX, R):
    """k_geneo_residual: R = CX - mu[sub] .* AX; mu a device tensor (nsub, m), the blocks (n, m) views"""
    m, (lda, ldc, ldr) = _block_ld(AX, CX, R)
    assert mu.is_contiguous() and mu.shape[1] == m
    _geneo_helper(ctx, 1, sub_ptr, m, R, ldr, a=AX, lda=lda, b=CX, ldb=ldc, s=mu)


def geneo_copy_cols(ctx: Context, sub_ptr, src, dst):
    m, (lds_, ldd) = _block_ld(src, dst)
    _geneo_helper(ctx, 2, sub_ptr, m, dst, ldd, a=src, lda=lds_)


def geneo_rowscale(ctx: Context, sub_ptr, w, X):
    m, (ld,) = _block_ld(X)
    _geneo_helper(ctx, 3, sub_ptr, m, X, ld, s=w)


def geneo_invsqrt_diag(ctx: Context, sub_ptr, G, s):
    """k_geneo_invsqrt_diag: s[sub, j] = 1 / sqrt(G[sub, j, j]), 0 for diagonals <= 1e-300; G (nsub, m, m), s (nsub, m) contiguous"""
    assert G.is_contiguous() and s.is_contiguous() and G.shape[1] == G.shape[2] == s.shape[1]
    _geneo_helper(ctx, 4, sub_ptr, G.shape[1], s, 0, a=G)


def geneo_finalize(ctx: Context, sub_ptr, scale, V, basis):
    """k_geneo_finalize: basis[j, i] = scale[sub(i), j] V[i, j] for j < nev = basis.shape[0]; scale (nsub, m), V an (n, m) view"""
    m, (ldv,) = _block_ld(V)
    assert scale.is_contiguous() and scale.shape[1] == m and basis.is_contiguous() and basis.shape[1] == V.shape[0]
    _geneo_helper(ctx, 5, sub_ptr, m, basis, 0, a=V, lda=ldv, s=scale, nev=basis.shape[0])


def geneo_start_block(ctx: Context, seed, mask, kept, S):
    """k_geneo_start_block as a warm eigensolver run launches it: S (n, 3m) contiguous from the first min(m_kept, m) columns of kept
    (n, m_kept) contiguous, the generator of geneo_random for the other columns of the X slot, zero W / P slots, zero rows where mask is 0"""
    assert S.is_contiguous() and kept.is_contiguous() and mask.is_contiguous() and S.shape[1] % 3 == 0
    assert S.shape[0] == kept.shape[0] == mask.shape[0]
    ctx.check(ctx.lib.ddm_geneo_debug_start_block(ctx.h, int(S.shape[0]), int(S.shape[1]) // 3, int(kept.shape[1]), int(seed), _ptr(mask), _ptr(kept), _ptr(S)))


def _csr_arrays(M):
    import scipy.sparse as sp
    M = sp.csr_matrix(M)
    if not M.has_sorted_indices:
        M = M.sorted_indices()
    return _np(M.indptr, np.int64), _np(M.indices, np.int32), _np(M.data, np.float64)


def geneo_pencil_host(A, B, pou, dirichlet=None, sigma=1e-3):
    """(rowptr, col, val_At, val_C, origin): the GenEO pencil A~ = A + sigma C~, C~ = D B D without Dirichlet rows / columns on the union
    pattern of two scipy CSR matrices, and its origin map (uint32 per entry: low half 1 + offset in A's row, high half 1 + offset in
    B's row, 0 = absent) -- the eigensolver's host assembly, no device needed"""
    lib = load_library()
    arp, aci, ava = _csr_arrays(A)
    brp, bci, bva = _csr_arrays(B)
    n = len(arp) - 1
    cap = max(len(aci) + len(bci), 1)
    rp, ci = np.empty(n + 1, dtype=np.int64), np.empty(cap, dtype=np.int32)
    vt, vc, org = np.empty(cap), np.empty(cap), np.empty(cap, dtype=np.uint32)
    nnz = ctypes.c_int64()
    pou = _np(pou, np.float64)
    dm = _np(dirichlet, np.uint8) if dirichlet is not None else None
    rc = lib.ddm_geneo_pencil_host(n, _hp(arp), _hp(aci), _hp(ava), _hp(brp), _hp(bci), _hp(bva), _hp(pou), _hp(dm) if dm is not None else None, float(sigma),
                                   _hp(rp), _hp(ci), _hp(vt), _hp(vc), _hp(org), ctypes.byref(nnz))
    if rc:
        raise ValueError(f"ddm_geneo_pencil_host: error {rc}")
    k = nnz.value
    return rp, ci[:k].copy(), vt[:k].copy(), vc[:k].copy(), org[:k].copy()


def geneo_pencil_refresh_host(rowptr, col, origin, A, B, pou, dirichlet=None, sigma=1e-3):
    """(val_At, val_C) of the pencil from the current values of A and B (same patterns as at assembly) through the origin map"""
    lib = load_library()
    arp, _, ava = _csr_arrays(A)
    brp, _, bva = _csr_arrays(B)
    rp, ci, org = _np(rowptr, np.int64), _np(col, np.int32), _np(origin, np.uint32)
    n = len(rp) - 1
    vt, vc = np.empty(max(len(ci), 1)), np.empty(max(len(ci), 1))
    pou = _np(pou, np.float64)
    dm = _np(dirichlet, np.uint8) if dirichlet is not None else None
    rc = lib.ddm_geneo_pencil_refresh_host(n, _hp(rp), _hp(ci), _hp(org), _hp(arp), _hp(ava), _hp(brp), _hp(bva), _hp(pou), _hp(dm) if dm is not None else None,
                                           float(sigma), _hp(vt), _hp(vc))
    if rc:
        raise ValueError(f"ddm_geneo_pencil_refresh_host: error {rc}")
    return vt[:len(ci)], vc[:len(ci)]
