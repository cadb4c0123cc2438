"""ctypes binding of include/fhesi_hip.h (the C ABI of the HIP library).

No compute happens in Python and there is no CPU fallback: if the shared library is missing or a HIP call fails,
the binding raises FhesiError with the library's message.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_DIR, "csrc")
_SO = os.environ.get("FHESI_LIB") or os.path.join(_CSRC, "libfhesi_hip.so")     # FHESI_LIB: dev override (ablation builds)

OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_SET = 0, 1, 2, 3, 4

# every symbol include/fhesi_hip.h declares (tests/test_abi.py checks the library exports all of them)
ABI_SYMBOLS = [
    "fhesi_last_error", "fhesi_device_count", "fhesi_ctx_create", "fhesi_ctx_destroy", "fhesi_ctx_m", "fhesi_ctx_phim",
    "fhesi_ctx_nprimes", "fhesi_ctx_prime", "fhesi_ctx_zms_idx", "fhesi_ctx_phi_m", "fhesi_ctx_sync", "fhesi_ctx_stream",
    "fhesi_timer_start", "fhesi_timer_stop", "fhesi_cmod_fft", "fhesi_cmod_ifft", "fhesi_dcrt_alloc", "fhesi_dcrt_free",
    "fhesi_dcrt_copy", "fhesi_dcrt_index_set", "fhesi_dcrt_equal", "fhesi_dcrt_upload_row", "fhesi_dcrt_download_row",
    "fhesi_dcrt_device_ptr", "fhesi_dcrt_from_poly", "fhesi_dcrt_to_poly", "fhesi_dcrt_op", "fhesi_dcrt_op_scalar",
    "fhesi_dcrt_automorph", "fhesi_dcrt_add_primes", "fhesi_dcrt_remove_primes", "fhesi_dcrt_from_scrt", "fhesi_dcrt_to_scrt",
    "fhesi_rows_ntt_fwd_dev", "fhesi_rows_ntt_inv_dev", "fhesi_rows_op_dev", "fhesi_ksk_create", "fhesi_ksk_free",
    "fhesi_ksk_upload", "fhesi_ksk_device_ptr", "fhesi_ksk_bytes", "fhesi_ct_mul_relin_batch", "fhesi_ct_mul_relin_batch_dev",
    "fhesi_ct_mul_dev", "fhesi_apply_key_switch_dev", "fhesi_dev_alloc", "fhesi_dev_free", "fhesi_dev_upload", "fhesi_dev_download",
    "fhesi_dev_copy", "fhesi_prof_enable", "fhesi_prof_read",
    "fhesi_ct_add_dev", "fhesi_ct_mul_long_dev", "fhesi_rows_mul_long_dev", "fhesi_ct_automorph_dev", "fhesi_ct_automorph_key_switch_dev",
    "fhesi_ct_gather_dev", "fhesi_ct_mul_sum_relin_dev", "fhesi_encrypt_batch", "fhesi_decrypt_batch", "fhesi_dcrt_exp", "fhesi_selftest_aux32",
    "fhesi_ctx_set_option", "fhesi_ctx_get_option", "fhesi_ctx_copy_options", "fhesi_host_alloc", "fhesi_host_free", "fhesi_ksk_key_bits", "fhesi_prof_kernel_name", "fhesi_ksk_mark_dirty", "fhesi_ksk_upload_dev",
    "fhesi_dcrt_add_primes_and_scale", "fhesi_dcrt_scale_down_to_set",
    "fhesi_keyswitch_init_batch", "fhesi_ksk_download", "fhesi_comm_init_all", "fhesi_comm_from_rccl", "fhesi_comm_destroy", "fhesi_comm_rank",
    "fhesi_comm_size", "fhesi_ksk_broadcast", "fhesi_comm_broadcast_dev", "fhesi_comm_exchange", "fhesi_comm_exchange_begin", "fhesi_comm_exchange_end", "fhesi_comm_allreduce_rows", "fhesi_scrt_alloc", "fhesi_scrt_from_poly", "fhesi_scrt_to_poly", "fhesi_scrt_op_scalar", "fhesi_dcrt_assign_scrt", "fhesi_scrt_assign_dcrt",
    "fhesi_ksk_form", "fhesi_ct_add_const_dev", "fhesi_ct_mul_poly_dev",
    "fhesi_encrypt_batch_seeded", "fhesi_keyswitch_init_batch_seeded", "fhesi_dcrt_sample",
    "fhesi_abi_version", "fhesi_host_stage_release",
    "fhesi_slots_plan", "fhesi_slots_create", "fhesi_slots_free", "fhesi_slots_info", "fhesi_slots_exponents", "fhesi_slots_embed", "fhesi_slots_decode",
    "fhesi_slots_embed_dev", "fhesi_slots_decode_dev", "fhesi_encrypt_slots_batch_seeded", "fhesi_decrypt_slots_batch", "fhesi_encrypt_noise_batch_seeded",
    "fhesi_slots_plan_pow2", "fhesi_slots_create_pow2", "fhesi_slots_shape", "fhesi_slots_set_path",
    "fhesi_slots_basis_plan", "fhesi_slots_basis_check", "fhesi_slots_basis_create", "fhesi_slots_basis_free", "fhesi_slots_basis_info", "fhesi_slots_basis_channel",
    "fhesi_slots_basis_embed", "fhesi_slots_basis_decode", "fhesi_slots_basis_embed_dev", "fhesi_slots_basis_decode_dev",
    "fhesi_encrypt_int_slots_batch_seeded", "fhesi_decrypt_int_slots_batch", "fhesi_encrypt_noise_int_batch_seeded",
    "fhesi_ctx_lin_class",
    "fhesi_plain_create_slots", "fhesi_plain_create_poly", "fhesi_plain_free", "fhesi_plain_info", "fhesi_plain_sum_bits", "fhesi_ct_plain_sum_dev", "fhesi_ct_add_slots_dev",
    "fhesi_ct_noise_batch", "fhesi_decrypt_noise_batch", "fhesi_ct_noise_int_batch",
    "fhesi_ksk_hoist", "fhesi_ct_rotations_dev", "fhesi_ct_matvec_dev",
    "fhesi_ct_rot_sum_dev", "fhesi_matvec_bsgs_plan", "fhesi_ct_matvec_bsgs_dev",
    "fhesi_linear_plan", "fhesi_linear_create", "fhesi_linear_create_dev", "fhesi_linear_free", "fhesi_linear_info", "fhesi_linear_diagonals",
    "fhesi_ct_rot_fold_dev", "fhesi_ct_linear_dev",
    "fhesi_linear_grid_plan", "fhesi_linear_grid_create", "fhesi_linear_grid_create_dev", "fhesi_linear_grid_free", "fhesi_linear_grid_info",
    "fhesi_linear_grid_diagonals", "fhesi_ct_linear_grid_dev",
    "fhesi_conv2d_plan", "fhesi_conv2d_create", "fhesi_conv2d_create_dev", "fhesi_conv2d_free", "fhesi_conv2d_info", "fhesi_conv2d_masks", "fhesi_ct_conv2d_dev",
    "fhesi_conv2d_lattice_plan", "fhesi_conv2d_lattice_create", "fhesi_conv2d_lattice_create_dev", "fhesi_conv2d_lattice_masks", "fhesi_conv2d_lattice_info",
    "fhesi_pool2d_plan", "fhesi_ct_pool2d_dev", "fhesi_slots_lattice_columns", "fhesi_slots_lattice_columns_dev",
    "fhesi_ct_lin_comb_dev", "fhesi_poly_eval_plan", "fhesi_ct_poly_eval_dev",
]
ROT_SUM_MAX_TERMS = 16   # FHESI_ROT_SUM_MAX_TERMS: the terms one launch of the rotated-sum kernel takes (more terms chain launches)
ABI_VERSION = 9          # FHESI_ABI_VERSION of the include/fhesi_hip.h this table was written against (checked in _load)
PROF_CLASSES = {"ntt_fwd": 0, "ntt_inv": 1, "rns_reduce": 2, "tensor": 3, "crt": 4, "digits": 5, "dot": 6, "ew": 7, "ntt_fwd_digits_main": 8,
                "plain_sum": 15}          # (numbered behind the name-only records below, which keep their public numbers)
# name-only records (Context.prof_kernel_name; no stopwatch, so not in PROF_CLASSES): the closing kernel the last profiled launch ran
# (class 13 is FHESI_PROF_NAME_DIGITS in the header; its key here is "digits_kernel" because prof_kernel_name takes the keys of both dictionaries
# and "digits" is the timed class 5 of PROF_CLASSES)
PROF_NAMES = {"crt_exact": 9, "ks_recombine": 10, "rns_generic": 11, "modswitch": 12, "digits_kernel": 13}


def _words_to_ints(words: np.ndarray) -> list:
    """[count][nw] little-endian 64-bit words -> Python integers"""
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in words]


class FhesiError(RuntimeError):
    pass


def library_path() -> str:
    return _SO


def build_library(force: bool = False) -> str:
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".cpp", ".h", ".inc"))]
    srcs.append(os.path.join(os.path.dirname(_DIR), "include", "fhesi_hip.h"))
    stale = force or not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", _CSRC, "-j8"], stdout=subprocess.DEVNULL)
    return _SO


_lib = None
_vp, _i32, _i64, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
_byref = C.byref         # (for functions whose parameters are named R and C, as the layers are)


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise FhesiError(f"HIP extension not built: {_SO} is missing (run __graft_entry__.build())")
    # One HIP runtime per process: PyTorch ships its own libamdhip64, the library links /opt/rocm's.  Whichever is loaded first
    # serves both (same soname); loading ours first and torch afterwards leaves torch without a device ("No HIP GPUs are
    # available").  So when torch is installed it is imported first -- it is only ever used for pool memory and collectives
    # (fhe-si_amd/regression.py, bench.py), never for compute.  FHESI_NO_TORCH_PRELOAD=1 skips this.
    if "torch" not in sys.modules and not os.environ.get("FHESI_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(_SO)
    lib.fhesi_last_error.restype = C.c_char_p
    # a library of another ABI revision would accept this table's calls and shift their arguments: refuse it
    have = lib.fhesi_abi_version() if hasattr(lib, "fhesi_abi_version") else None
    if have != ABI_VERSION:
        raise FhesiError(f"{_SO} has ABI revision {have}, this binding was written against {ABI_VERSION}: rebuild (make -C fhe-si_amd/csrc)")
    sig = {
        "fhesi_device_count": [_vp],
        "fhesi_ctx_create": [_vp, _i64, _i32, _vp, _vp, _i32],
        "fhesi_ctx_destroy": [_vp],
        "fhesi_ctx_prime": [_vp, _i32, _vp, _vp],
        "fhesi_ctx_zms_idx": [_vp, _vp],
        "fhesi_ctx_phi_m": [_vp, _vp],
        "fhesi_ctx_sync": [_vp],
        "fhesi_ctx_lin_class": [_vp, _i64, _vp, _vp, _vp],
        "fhesi_timer_start": [_vp],
        "fhesi_timer_stop": [_vp, _vp],
        "fhesi_cmod_fft": [_vp, _i32, _vp, _i32, _i64, _vp],
        "fhesi_cmod_ifft": [_vp, _i32, _vp, _vp],
        "fhesi_dcrt_alloc": [_vp, _vp, _i32, _vp],
        "fhesi_dcrt_free": [_vp],
        "fhesi_dcrt_copy": [_vp, _vp],
        "fhesi_dcrt_index_set": [_vp, _vp, _vp],
        "fhesi_dcrt_equal": [_vp, _vp, _vp],
        "fhesi_dcrt_upload_row": [_vp, _i32, _vp],
        "fhesi_dcrt_download_row": [_vp, _i32, _vp],
        "fhesi_dcrt_from_poly": [_vp, _vp, _i32, _i64],
        "fhesi_dcrt_to_poly": [_vp, _vp, _i32, _i32, _vp, _i32],
        "fhesi_dcrt_op": [_vp, _vp, _i32],
        "fhesi_dcrt_op_scalar": [_vp, _vp, _i32, _i32],
        "fhesi_dcrt_automorph": [_vp, _i64],
        "fhesi_dcrt_exp": [_vp, _i64],
        "fhesi_selftest_aux32": [_vp],
        "fhesi_dcrt_add_primes": [_vp, _vp, _i32],
        "fhesi_dcrt_remove_primes": [_vp, _vp, _i32],
        "fhesi_dcrt_from_scrt": [_vp, _vp],
        "fhesi_dcrt_to_scrt": [_vp, _vp],
        "fhesi_rows_ntt_fwd_dev": [_vp, _vp, _i64],
        "fhesi_rows_ntt_inv_dev": [_vp, _vp, _i64],
        "fhesi_rows_op_dev": [_vp, _vp, _vp, _i64, _i32],
        "fhesi_ksk_create": [_vp, _i32, _i32, _vp],
        "fhesi_ksk_free": [_vp],
        "fhesi_ksk_upload": [_vp, _vp],
        "fhesi_ct_mul_relin_batch": [_vp, _vp, _i32, _u64, _i32, _vp, _vp, _vp, _i32, _i64],
        "fhesi_ct_mul_relin_batch_dev": [_vp, _vp, _i32, _u64, _i32, _vp, _vp, _vp, _i32, _i64],
        "fhesi_ct_mul_dev": [_vp, _u64, _vp, _vp, _i32, _i64, _vp],
        "fhesi_apply_key_switch_dev": [_vp, _vp, _i32, _i32, _vp, _i64, _vp, _i32],
        "fhesi_ct_add_dev": [_vp, _i32, _vp, _vp, _i32, _i32, _i64],
        "fhesi_ct_mul_long_dev": [_vp, _i32, _vp, _i64, _i32, _i32, _i64],
        "fhesi_rows_mul_long_dev": [_vp, _vp, _i64, _i64],
        "fhesi_ct_automorph_dev": [_vp, _i64, _vp, _i32, _i32, _i64, _vp, _i32],
        "fhesi_ct_automorph_key_switch_dev": [_vp, _vp, _i32, _i32, _i64, _vp, _i32, _i64, _vp, _i32],
        "fhesi_ct_gather_dev": [_vp, _vp, _vp, _i64, _i64, _vp],
        "fhesi_ct_mul_sum_relin_dev": [_vp, _vp, _i32, _u64, _i32, _vp, _i32, _vp, _vp, _vp, _i64, _vp],
        "fhesi_encrypt_batch": [_vp, _vp, _vp, _i32, _u64, _vp, _vp, _i64, _vp, _i32],
        "fhesi_decrypt_batch": [_vp, _vp, _i32, _u64, _vp, _i32, _i64, _vp],
        "fhesi_dev_alloc": [_vp, C.c_size_t, _vp],
        "fhesi_dev_free": [_vp, _vp],
        "fhesi_dev_upload": [_vp, _vp, _vp, C.c_size_t],
        "fhesi_dev_download": [_vp, _vp, _vp, C.c_size_t],
        "fhesi_dev_copy": [_vp, _vp, _vp, C.c_size_t],
        "fhesi_prof_enable": [_vp, _i32],
        "fhesi_prof_read": [_vp, _i32, _vp, _vp, _vp],
        "fhesi_prof_kernel_name": [_vp, _i32, _vp, C.c_size_t],
        "fhesi_ctx_set_option": [_vp, C.c_char_p, _i64],
        "fhesi_ctx_get_option": [_vp, C.c_char_p, _vp],
        "fhesi_ctx_copy_options": [_vp, _vp],
        "fhesi_host_alloc": [_vp, C.c_size_t, _vp],
        "fhesi_host_free": [_vp, _vp],
        "fhesi_host_stage_release": [_vp],
        "fhesi_ksk_key_bits": [_vp, _vp, _vp],
        "fhesi_ksk_mark_dirty": [_vp],
        "fhesi_comm_init_all": [_i32, _vp, _vp],
        "fhesi_comm_from_rccl": [_vp, _vp],
        "fhesi_comm_destroy": [_vp],
        "fhesi_ksk_broadcast": [_vp, _vp, _i32],
        "fhesi_comm_broadcast_dev": [_vp, _vp, _vp, C.c_size_t, _i32],
        "fhesi_comm_exchange": [_vp, _vp, _vp, _vp],
        "fhesi_comm_exchange_begin": [_vp, _vp, _vp, _vp],
        "fhesi_comm_exchange_end": [_vp, _vp],
        "fhesi_comm_allreduce_rows": [_vp, _vp, _vp, _i64],
        "fhesi_ksk_download": [_vp, _vp],
        "fhesi_keyswitch_init_batch": [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp],
        "fhesi_scrt_alloc": [_vp, _vp, _i32, _vp],
        "fhesi_scrt_from_poly": [_vp, _vp, _i32, _i64],
        "fhesi_scrt_to_poly": [_vp, _vp, _i32, _vp, _i32],
        "fhesi_scrt_op_scalar": [_vp, _vp, _i32, _i32],
        "fhesi_dcrt_assign_scrt": [_vp, _vp],
        "fhesi_scrt_assign_dcrt": [_vp, _vp, _vp, _i32],
        "fhesi_dcrt_add_primes_and_scale": [_vp, _vp, _i32, _u64, _vp],
        "fhesi_dcrt_scale_down_to_set": [_vp, _vp, _i32, _u64],
        "fhesi_ksk_upload_dev": [_vp, _vp],
        "fhesi_ksk_form": [_vp, _vp, _vp, _vp],
        "fhesi_encrypt_batch_seeded": [_vp, _vp, _vp, _i32, _u64, _u64, _u64, _vp, _i64, _vp, _i32],
        "fhesi_keyswitch_init_batch_seeded": [_vp, _vp, _i32, _vp, _i32, _i32, _u64, _u64, _u64],
        "fhesi_dcrt_sample": [_vp, _i32, _i64, _u64, _u64],
        "fhesi_ct_add_const_dev": [_vp, _i32, _u64, _vp, _i32, _i32, _i64, _vp, _i32],
        "fhesi_ct_mul_poly_dev": [_vp, _i32, _vp, _i32, _i32, _i64, _vp, _i32],
        "fhesi_slots_plan": [_i64, _u64, _i64, _vp, _vp, _vp, _vp, _vp],
        "fhesi_slots_create": [_vp, _u64, _i64, _vp],
        "fhesi_slots_free": [_vp],
        "fhesi_slots_info": [_vp, _vp, _vp, _vp, _vp],
        "fhesi_slots_exponents": [_vp, _vp],
        "fhesi_slots_embed": [_vp, _vp, _i64, _i32, _i64, _vp],
        "fhesi_slots_decode": [_vp, _vp, _i64, _i64, _i32, _vp],
        "fhesi_slots_embed_dev": [_vp, _vp, _i64, _i32, _i64, _vp],
        "fhesi_slots_decode_dev": [_vp, _vp, _i64, _i64, _i32, _vp],
        "fhesi_encrypt_slots_batch_seeded": [_vp, _vp, _vp, _vp, _i32, _u64, _u64, _vp, _i64, _i32, _i64, _vp, _i32],
        "fhesi_decrypt_slots_batch": [_vp, _vp, _vp, _i32, _vp, _i32, _i64, _i64, _i32, _vp],
        "fhesi_encrypt_noise_batch_seeded": [_vp, _vp, _vp, _vp, _i32, _u64, _u64, _i64, _vp, _i32],
        "fhesi_slots_plan_pow2": [_i64, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
        "fhesi_slots_create_pow2": [_vp, _u64, _i64, _vp],
        "fhesi_slots_shape": [_vp, _vp, _vp, _vp],
        "fhesi_slots_set_path": [_vp, _i32],
        "fhesi_slots_basis_plan": [_i64, _i32, _i32, _i64, _vp, _vp, _vp],
        "fhesi_slots_basis_check": [_i64, _vp, _i32, _i64, _vp, _vp],
        "fhesi_slots_basis_create": [_vp, _vp, _i32, _i64, _vp],
        "fhesi_slots_basis_free": [_vp],
        "fhesi_slots_basis_info": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "fhesi_slots_basis_channel": [_vp, _i32, _vp],
        "fhesi_slots_basis_embed": [_vp, _vp, _i32, _i64, _i64, _vp],
        "fhesi_slots_basis_decode": [_vp, _vp, _i64, _i64, _vp],
        "fhesi_slots_basis_embed_dev": [_vp, _vp, _i32, _i64, _i64, _vp],
        "fhesi_slots_basis_decode_dev": [_vp, _vp, _i64, _i64, _vp],
        "fhesi_encrypt_int_slots_batch_seeded": [_vp, _vp, _vp, _vp, _i32, _u64, _u64, _vp, _i32, _i64, _i64, _vp, _i32],
        "fhesi_decrypt_int_slots_batch": [_vp, _vp, _vp, _i32, _vp, _i32, _i64, _i64, _vp],
        "fhesi_encrypt_noise_int_batch_seeded": [_vp, _vp, _vp, _vp, _i32, _u64, _u64, _i64, _vp, _i32],
        "fhesi_plain_create_slots": [_vp, _vp, _i64, _i32, _i64, _vp],
        "fhesi_plain_create_poly": [_vp, _vp, _i64, _vp],
        "fhesi_plain_free": [_vp],
        "fhesi_plain_info": [_vp, _vp, _vp, _vp],
        "fhesi_plain_sum_bits": [_i64, _i32, _u64, _i64, _vp],
        "fhesi_ct_plain_sum_dev": [_vp, _vp, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp],
        "fhesi_ct_add_slots_dev": [_vp, _vp, _i32, _vp, _i32, _i32, _i64, _vp, _i64, _i32, _i64],
        "fhesi_ct_noise_batch": [_vp, _vp, _i32, _u64, _vp, _i32, _i64, _vp, _vp],
        "fhesi_decrypt_noise_batch": [_vp, _vp, _i32, _u64, _vp, _i32, _i64, _vp, _vp, _vp],
        "fhesi_ct_noise_int_batch": [_vp, _vp, _vp, _i32, _vp, _i32, _i64, _vp],
        "fhesi_ksk_hoist": [_vp, _i64, _vp],
        "fhesi_ct_rotations_dev": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i64, _vp, _i32],
        "fhesi_ct_matvec_dev": [_vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _vp],
        "fhesi_ct_rot_sum_dev": [_vp, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _vp],
        "fhesi_matvec_bsgs_plan": [_i64, _vp, _vp],
        "fhesi_ct_matvec_bsgs_dev": [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _vp],
        "fhesi_linear_plan": [_i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
        "fhesi_linear_create": [_vp, _vp, _i64, _i64, _vp, _i32, _vp],
        "fhesi_linear_create_dev": [_vp, _vp, _i64, _i64, _vp, _i32, _vp],
        "fhesi_linear_free": [_vp],
        "fhesi_linear_info": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "fhesi_linear_diagonals": [_vp, _vp, _i64, _i64, _i32, _vp],
        "fhesi_ct_rot_fold_dev": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i64, _vp],
        "fhesi_ct_linear_dev": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i64, _vp],
        "fhesi_linear_grid_plan": [_i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "fhesi_linear_grid_create": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _i32, _vp],
        "fhesi_linear_grid_create_dev": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _i32, _vp],
        "fhesi_linear_grid_free": [_vp],
        "fhesi_linear_grid_info": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "fhesi_linear_grid_diagonals": [_vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp],
        "fhesi_ct_linear_grid_dev": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i64, _vp],
        "fhesi_conv2d_plan": [_i64] * 9 + [_i32, _vp, _vp, _vp, _vp, _vp],
        "fhesi_conv2d_create": [_vp, _vp] + [_i64] * 8 + [_vp, _i32, _vp],
        "fhesi_conv2d_create_dev": [_vp, _vp] + [_i64] * 8 + [_vp, _i32, _vp],
        "fhesi_conv2d_free": [_vp],
        "fhesi_conv2d_info": [_vp] * 15,
        "fhesi_conv2d_masks": [_vp, _vp] + [_i64] * 8 + [_i32, _vp],
        "fhesi_ct_conv2d_dev": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i64, _vp],
        "fhesi_conv2d_lattice_plan": [_i64] * 15 + [_i32] + [_vp] * 7,
        "fhesi_conv2d_lattice_create": [_vp, _vp] + [_i64] * 14 + [_vp, _i32, _vp],
        "fhesi_conv2d_lattice_create_dev": [_vp, _vp] + [_i64] * 14 + [_vp, _i32, _vp],
        "fhesi_conv2d_lattice_masks": [_vp, _vp] + [_i64] * 14 + [_i32, _vp],
        "fhesi_conv2d_lattice_info": [_vp] * 9,
        "fhesi_pool2d_plan": [_i64] * 7 + [_i32] + [_vp] * 8,
        "fhesi_ct_pool2d_dev": [_vp] + [_i64] * 6 + [_i32, _vp, _i32, _i32, _i32, _vp, _i32, _i64, _vp],
        "fhesi_slots_lattice_columns": [_vp, _vp] + [_i64] * 6 + [_vp],
        "fhesi_slots_lattice_columns_dev": [_vp, _vp] + [_i64] * 6 + [_vp],
        "fhesi_ct_lin_comb_dev": [_vp, _i32, _u64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _vp],
        "fhesi_poly_eval_plan": [_i32, _i32, _vp, _vp, _vp, _vp, _vp],
        "fhesi_ct_poly_eval_dev": [_vp, _vp, _i32, _u64, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _vp],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    for name in ("fhesi_ctx_m", "fhesi_ctx_phim"):
        getattr(lib, name).argtypes = [_vp]
        getattr(lib, name).restype = _i64
    lib.fhesi_ctx_nprimes.argtypes = [_vp]
    lib.fhesi_ctx_nprimes.restype = _i32
    for name in ("fhesi_ctx_stream", "fhesi_dcrt_device_ptr", "fhesi_ksk_device_ptr"):
        getattr(lib, name).argtypes = [_vp]
        getattr(lib, name).restype = _vp
    for name in ("fhesi_comm_rank", "fhesi_comm_size"):
        getattr(lib, name).argtypes = [_vp]
        getattr(lib, name).restype = _i32
    lib.fhesi_ksk_bytes.argtypes = [_vp]
    lib.fhesi_ksk_bytes.restype = C.c_size_t
    _lib = lib
    return lib


def _ck(rc: int):
    if rc != 0:
        raise FhesiError(_load().fhesi_last_error().decode())


def _p(a: np.ndarray):
    return a.ctypes.data_as(_vp)


def lin_class(m: int, ctx: "Context" = None):
    """-> (offset, stride, lin_lg): the fold of the rings m = q^k, 2 q^k (q an odd prime) on the fused 30-bit paths, as a context on m would
    take it (or as `ctx` took it); (0, 0, 0) for any other m.  Touches no device."""
    off, st, lg = _i64(0), _i64(0), _i32(0)
    _ck(_load().fhesi_ctx_lin_class(ctx.h if ctx is not None else None, int(m), C.byref(off), C.byref(st), C.byref(lg)))
    return off.value, st.value, lg.value


class Backend:
    @staticmethod
    def lib():
        return _load()

    @staticmethod
    def device_count() -> int:
        n = _i32(0)
        _ck(_load().fhesi_device_count(C.byref(n)))
        return n.value


class DevBuf:
    """Plain HBM buffer owned through the C ABI."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = _vp()
        _ck(_load().fhesi_dev_alloc(ctx.h, nbytes, C.byref(self.ptr)))

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _ck(_load().fhesi_dev_upload(self.ctx.h, self.ptr, _p(arr), arr.nbytes))
        return self

    def download(self, shape, dtype=np.uint64) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _ck(_load().fhesi_dev_download(self.ctx.h, _p(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            _load().fhesi_dev_free(self.ctx.h, self.ptr)
            self.ptr = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """FHEcontext + Cmodulus chain on one GPU (fhesi_ctx_create)."""

    def __init__(self, m: int, primes, roots, device: int = 0):
        q = np.array([int(x) for x in primes], dtype=np.uint64)
        r = np.array([int(x) for x in roots], dtype=np.uint64)
        self.h = _vp()
        _ck(_load().fhesi_ctx_create(C.byref(self.h), m, len(q), _p(q), _p(r), device))
        self.m, self.primes, self.roots = m, [int(x) for x in q], [int(x) for x in r]
        self.L = len(self.primes)
        self.phim = _load().fhesi_ctx_phim(self.h)

    def close(self):
        if getattr(self, "h", None):
            _load().fhesi_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _ck(_load().fhesi_ctx_sync(self.h))

    def zms_idx(self) -> np.ndarray:
        out = np.zeros(self.m, dtype=np.int32)
        _ck(_load().fhesi_ctx_zms_idx(self.h, _p(out)))
        return out

    def phi_m(self) -> np.ndarray:
        out = np.zeros(self.phim + 1, dtype=np.int64)
        _ck(_load().fhesi_ctx_phi_m(self.h, _p(out)))
        return out

    def lin_class(self):
        """-> (offset, stride, lin_lg) of the linear-convolution class this context took ((0, 0, 0): negacyclic or per-prime rows)."""
        return lin_class(self.m, self)

    def timer_start(self):
        _ck(_load().fhesi_timer_start(self.h))

    def timer_stop(self) -> float:
        ms = C.c_float(0)
        _ck(_load().fhesi_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def prof_enable(self, on: bool = True):
        _ck(_load().fhesi_prof_enable(self.h, int(on)))

    def prof_read(self, cls: str):
        """-> (launches, units, total_ms) for one kernel class of PROF_CLASSES."""
        n, u, ms = _i64(0), C.c_double(0), C.c_double(0)
        _ck(_load().fhesi_prof_read(self.h, PROF_CLASSES[cls], C.byref(n), C.byref(u), C.byref(ms)))
        return n.value, u.value, ms.value

    def prof_kernel_name(self, cls: str) -> str:
        """Demangled name of the kernel the last profiled launch of that class (of PROF_CLASSES or PROF_NAMES) ran ('' if none)."""
        buf = C.create_string_buffer(512)
        _ck(_load().fhesi_prof_kernel_name(self.h, PROF_CLASSES[cls] if cls in PROF_CLASSES else PROF_NAMES[cls], buf, 512))
        return buf.value.decode()

    def set_option(self, name: str, value: int):
        _ck(_load().fhesi_ctx_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = _i64(0)
        _ck(_load().fhesi_ctx_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def selftest_aux32(self):
        """Diagnostic of the 32-bit auxiliary transforms of the key switch (n = 2^14): raises FhesiError on failure."""
        _ck(_load().fhesi_selftest_aux32(self.h))

    def dev_copy(self, dst_ptr: int, src_ptr: int, nbytes: int):
        _ck(_load().fhesi_dev_copy(self.h, _vp(dst_ptr), _vp(src_ptr), nbytes))

    # Cmodulus::FFT / iFFT
    def cmod_fft(self, prime: int, limbs: np.ndarray) -> np.ndarray:
        limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
        y = np.zeros(self.phim, dtype=np.uint64)
        _ck(_load().fhesi_cmod_fft(self.h, prime, _p(limbs), limbs.shape[1], limbs.shape[0], _p(y)))
        return y

    def cmod_ifft(self, prime: int, y: np.ndarray) -> np.ndarray:
        y = np.ascontiguousarray(y, dtype=np.uint64)
        x = np.zeros(self.phim, dtype=np.uint64)
        _ck(_load().fhesi_cmod_ifft(self.h, prime, _p(y), _p(x)))
        return x

    def alloc(self, nbytes: int) -> DevBuf:
        return DevBuf(self, nbytes)

    def upload(self, arr: np.ndarray) -> DevBuf:
        arr = np.ascontiguousarray(arr)
        return DevBuf(self, max(arr.nbytes, 8)).upload(arr)

    # batched device-resident rows [count][L][phim]
    def rows_ntt_fwd(self, buf: DevBuf, count: int):
        _ck(_load().fhesi_rows_ntt_fwd_dev(self.h, buf.ptr, count))

    def rows_ntt_inv(self, buf: DevBuf, count: int):
        _ck(_load().fhesi_rows_ntt_inv_dev(self.h, buf.ptr, count))

    def rows_op(self, dst: DevBuf, src: DevBuf, count: int, op: int):
        _ck(_load().fhesi_rows_op_dev(self.h, dst.ptr, src.ptr, count, op))

    def ct_mul_dev(self, p: int, a: DevBuf, b: DevBuf, nlimbs: int, count: int, tprod: DevBuf):
        _ck(_load().fhesi_ct_mul_dev(self.h, p, a.ptr, b.ptr, nlimbs, count, tprod.ptr))

    def apply_key_switch_dev(self, ksk: "KeySwitchMatrix", logQ: int, tprod: DevBuf, count: int, out: DevBuf, nlimbs: int, decomp_bytes: int = 3):
        _ck(_load().fhesi_apply_key_switch_dev(self.h, ksk.h, logQ, decomp_bytes, tprod.ptr, count, out.ptr, nlimbs))

    # ---- Encrypt / Decrypt batches (FHE-SI.cpp:10-36, 93-119); randomness supplied by the caller
    def encrypt_batch(self, pk0: "DoubleCRT", pk1: "DoubleCRT", logQ: int, p: int, rand: np.ndarray, msg: np.ndarray, out: DevBuf, nlimbs: int):
        """rand: [count][3][phim] int64 = (r, e0, e1); msg: [count][phim] int64; out: device [count][2][phim][nlimbs]."""
        rand = np.ascontiguousarray(rand, dtype=np.int64)
        msg = np.ascontiguousarray(msg, dtype=np.int64)
        assert rand.shape[0] == msg.shape[0] and rand.shape[1] == 3
        _ck(_load().fhesi_encrypt_batch(self.h, pk0.h, pk1.h, logQ, p, _p(rand), _p(msg), msg.shape[0], out.ptr, nlimbs))

    def encrypt_batch_seeded(self, pk0: "DoubleCRT", pk1: "DoubleCRT", logQ: int, p: int, seed: int, first_index: int, msg: np.ndarray, out: DevBuf, nlimbs: int):
        """FHESIPubKey::Encrypt with r, e0, e1 drawn on the device from (seed, first_index + i) -- philox.h."""
        msg = np.ascontiguousarray(msg, dtype=np.int64)
        _ck(_load().fhesi_encrypt_batch_seeded(self.h, pk0.h, pk1.h, logQ, p, seed, first_index, _p(msg), msg.shape[0], out.ptr, nlimbs))

    def decrypt_batch(self, sk1: "DoubleCRT", logQ: int, p: int, ct: DevBuf, nlimbs: int, count: int) -> np.ndarray:
        msg = np.zeros((count, self.phim), dtype=np.int64)
        _ck(_load().fhesi_decrypt_batch(self.h, sk1.h, logQ, p, ct.ptr, nlimbs, count, _p(msg)))
        return msg

    # ---- the noise budget of unscaled two-part ciphertexts (include/fhesi_hip.h: what is and is not measured)
    def noise_budget(self, sk1: "DoubleCRT", logQ: int, p: int, ct: DevBuf, nlimbs: int, count: int, maxres: bool = False):
        """budget [count] int32 = max(0, logQ - bitlen(max |residual|)); with maxres=True also the exact maxima as Python integers."""
        budget = np.zeros(count, dtype=np.int32)
        words = np.zeros((count, (logQ + 64) // 64), dtype=np.uint64) if maxres else None
        _ck(_load().fhesi_ct_noise_batch(self.h, sk1.h, logQ, p, ct.ptr, nlimbs, count, _p(budget), _p(words) if maxres else None))
        return (budget, _words_to_ints(words)) if maxres else budget

    def decrypt_noise_batch(self, sk1: "DoubleCRT", logQ: int, p: int, ct: DevBuf, nlimbs: int, count: int, maxres: bool = False):
        """(msg, budget[, maxres]) from one pass: msg is decrypt_batch's bit for bit."""
        msg = np.zeros((count, self.phim), dtype=np.int64)
        budget = np.zeros(count, dtype=np.int32)
        words = np.zeros((count, (logQ + 64) // 64), dtype=np.uint64) if maxres else None
        _ck(_load().fhesi_decrypt_noise_batch(self.h, sk1.h, logQ, p, ct.ptr, nlimbs, count, _p(msg), _p(budget), _p(words) if maxres else None))
        return (msg, budget, _words_to_ints(words)) if maxres else (msg, budget)

    # ---- ciphertext algebra between multiplications (Matrix<Ciphertext> / Regression), batches resident in HBM
    def ct_add_dev(self, logQ: int, dst: DevBuf, src: DevBuf, nparts: int, nlimbs: int, count: int):
        _ck(_load().fhesi_ct_add_dev(self.h, logQ, dst.ptr, src.ptr, nparts, nlimbs, count))

    def ct_mul_long_dev(self, logQ: int, ct: DevBuf, l: int, nparts: int, nlimbs: int, count: int):
        _ck(_load().fhesi_ct_mul_long_dev(self.h, logQ, ct.ptr, l, nparts, nlimbs, count))

    def ct_add_const_dev(self, logQ: int, p: int, ct: DevBuf, nparts: int, nlimbs: int, count: int, poly: np.ndarray):
        """Ciphertext::operator+=(const ZZX&) on unscaled ciphertexts (Ciphertext.cpp:147-156); poly [npoly][phim] int64, npoly 1 or count."""
        poly = np.ascontiguousarray(poly, dtype=np.int64).reshape(-1, self.phim)
        _ck(_load().fhesi_ct_add_const_dev(self.h, logQ, p, ct.ptr, nparts, nlimbs, count, _p(poly), poly.shape[0]))

    def ct_mul_poly_dev(self, logQ: int, ct: DevBuf, nparts: int, nlimbs: int, count: int, poly: np.ndarray):
        """Ciphertext::operator*=(const ZZX&) on unscaled ciphertexts (Ciphertext.cpp:245-249, :29-36)."""
        poly = np.ascontiguousarray(poly, dtype=np.int64).reshape(-1, self.phim)
        _ck(_load().fhesi_ct_mul_poly_dev(self.h, logQ, ct.ptr, nparts, nlimbs, count, _p(poly), poly.shape[0]))

    def rows_mul_long_dev(self, rows: DevBuf, l: int, count: int):
        _ck(_load().fhesi_rows_mul_long_dev(self.h, rows.ptr, l, count))

    def ct_automorph_dev(self, k: int, src: DevBuf, nparts: int, nlimbs_in: int, count: int, out: DevBuf, nlimbs_out: int):
        _ck(_load().fhesi_ct_automorph_dev(self.h, k, src.ptr, nparts, nlimbs_in, count, out.ptr, nlimbs_out))

    def ct_automorph_key_switch_dev(self, ksk: "KeySwitchMatrix", logQ: int, k: int, src: DevBuf, nlimbs_in: int, count: int, out: DevBuf,
                                    nlimbs: int, decomp_bytes: int = 3):
        _ck(_load().fhesi_ct_automorph_key_switch_dev(self.h, ksk.h, logQ, decomp_bytes, k, src.ptr, nlimbs_in, count, out.ptr, nlimbs))

    def ct_gather_dev(self, pool: DevBuf, idx, words: int, out: DevBuf):
        ia = np.ascontiguousarray(idx, dtype=np.int32)
        _ck(_load().fhesi_ct_gather_dev(self.h, pool.ptr, _p(ia), len(ia), words, out.ptr))

    def ct_mul_sum_relin_dev(self, ksk: "KeySwitchMatrix", logQ: int, p: int, pool: DevBuf, nlimbs: int, a_idx, b_idx, seg, out: DevBuf,
                             decomp_bytes: int = 3):
        """out[g] = KeySwitch(sum_{t in [seg[g], seg[g+1])} pool[a_idx[t]] * pool[b_idx[t]]): one wave of Matrix<Ciphertext> products."""
        ia, ib = np.ascontiguousarray(a_idx, dtype=np.int32), np.ascontiguousarray(b_idx, dtype=np.int32)
        sg = np.ascontiguousarray(seg, dtype=np.int32)
        assert len(ia) == len(ib) == int(sg[-1]) and sg[0] == 0
        _ck(_load().fhesi_ct_mul_sum_relin_dev(self.h, ksk.h, logQ, p, decomp_bytes, pool.ptr, nlimbs, _p(ia), _p(ib), _p(sg), len(sg) - 1, out.ptr))

    def ct_mul_relin_dev(self, ksk: "KeySwitchMatrix", logQ: int, p: int, a: DevBuf, b: DevBuf, out: DevBuf, nlimbs: int, count: int, decomp_bytes: int = 3):
        _ck(_load().fhesi_ct_mul_relin_batch_dev(self.h, ksk.h, logQ, p, decomp_bytes, a.ptr, b.ptr, out.ptr, nlimbs, count))

    def ct_mul_relin(self, ksk: "KeySwitchMatrix", logQ: int, p: int, a: np.ndarray, b: np.ndarray, decomp_bytes: int = 3, out: np.ndarray = None) -> np.ndarray:
        """a, b: [count][2][phim][nlimbs] uint64 two's complement -> same shape (host buffers: fhesi_ct_mul_relin_batch).  `out`: a result
        array to reuse (a fresh numpy array costs a page fault per 4 KiB on first touch); arrays from host_array() are pinned and take the
        DMA path without the staging copy."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        if out is None:
            out = np.empty_like(a)
        elif out.shape != a.shape or out.dtype != np.uint64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous uint64 array of the operands' shape")
        _ck(_load().fhesi_ct_mul_relin_batch(self.h, ksk.h, logQ, p, decomp_bytes, _p(a), _p(b), _p(out), a.shape[-1], a.shape[0]))
        return out

    def host_array(self, shape, dtype=np.uint64) -> np.ndarray:
        """numpy array over PINNED host memory (fhesi_host_alloc); freed when the array (and its views) are collected."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = _vp()
        _ck(_load().fhesi_host_alloc(self.h, n, C.byref(ptr)))
        buf = (C.c_char * max(n, 1)).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        import weakref
        # (the finalizer holds no context handle: fhesi_host_free does not dereference it, so the array may outlive the Context -- at
        # interpreter shutdown the order of collection is arbitrary)
        lib, addr = _load(), ptr.value
        weakref.finalize(buf, lambda: lib.fhesi_host_free(None, C.c_void_p(addr)))
        return arr

    # ---- prepared plaintext operands (fhesi_plain): sums of ciphertext x plaintext products
    def plain_from_poly(self, poly: np.ndarray) -> "Plain":
        """poly [nw][phim] signed int64 coefficient polynomials (the operand of Ciphertext *= ZZX) -> a prepared handle."""
        poly = np.ascontiguousarray(poly, dtype=np.int64).reshape(-1, self.phim)
        h = _vp()
        _ck(_load().fhesi_plain_create_poly(self.h, _p(poly), poly.shape[0], C.byref(h)))
        return Plain(self, h)

    def ct_plain_sum_dev(self, plain: "Plain", logQ: int, pool: DevBuf, npool: int, nlimbs: int, a_idx, b_idx, seg, out: DevBuf):
        """out[g] = sum_{t in [seg[g], seg[g+1])} pool[a_idx[t]] (*) plain[b_idx[t]] on unscaled two-part ciphertexts; the arguments are checked
        by the library (FhesiError names what it refuses)."""
        ia, ib = np.ascontiguousarray(a_idx, dtype=np.int32), np.ascontiguousarray(b_idx, dtype=np.int32)
        sg = np.ascontiguousarray(seg, dtype=np.int32)
        _ck(_load().fhesi_ct_plain_sum_dev(self.h, plain.h, logQ, pool.ptr, npool, nlimbs, _p(ia), _p(ib), _p(sg), len(sg) - 1, out.ptr))

    # ---- hoisted rotations: many automorphism key switches of one ciphertext (fhesi_ct_rotations_dev)
    @staticmethod
    def _hoisted_args(hoisted, ks):
        ks = [int(k) for k in ks]
        if len(hoisted) != len(ks):
            raise ValueError("one matrix (or None, the identity) per k")
        hs = (_vp * max(len(ks), 1))(*[h.h if h is not None else None for h in hoisted])
        return hs, np.ascontiguousarray(ks, dtype=np.int64)

    def ct_rotations_dev(self, hoisted, ks, logQ: int, src: DevBuf, nlimbs_in: int, count: int, out: DevBuf, nlimbs: int, decomp_bytes: int = 3):
        """out[t][i] = Reduce((ApplyKeySwitch(hoisted[t], src[i])) >>= ks[t]): the rotations of every ciphertext by every k, the digits of a
        ciphertext made once.  hoisted[t]: KeySwitchMatrix.hoist(ks[t]) of the matrix of the automorphism ks[t], or None with ks[t] = 1 (the
        reduced copy).  out: [len(ks)][count][2][phim][nlimbs].  The library checks the arguments (FhesiError names what it refuses)."""
        hs, ka = self._hoisted_args(hoisted, ks)
        _ck(_load().fhesi_ct_rotations_dev(self.h, hs, _p(ka), len(ka), logQ, decomp_bytes, src.ptr, nlimbs_in, count, out.ptr, nlimbs))

    def ct_matvec_dev(self, hoisted, ks, plain: "Plain", logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """out[i] = sum_t rot_t(src[i]) (*) plain[t]: ct_rotations_dev into a workspace pool, then ct_plain_sum_dev -- those calls' bits."""
        hs, ka = self._hoisted_args(hoisted, ks)
        _ck(_load().fhesi_ct_matvec_dev(self.h, hs, _p(ka), len(ka), plain.h, logQ, decomp_bytes, src.ptr, nlimbs, count, out.ptr))

    # ---- baby-step/giant-step matrix-vector products (fhesi_ct_rot_sum_dev, fhesi_ct_matvec_bsgs_dev)
    def ct_rot_sum_dev(self, ks, logQ: int, base, pre: DevBuf, count: int, nlimbs: int, out: DevBuf):
        """out[i] = Reduce(base[i] + sum_t (pre[t][i] >>= ks[t])): pre [len(ks)][count][2][phim][nlimbs]; base a buffer of count ciphertexts or None;
        out may be base.  The words of ct_automorph_dev per term, ct_add_dev and the reduction."""
        ka = np.ascontiguousarray([int(k) for k in ks], dtype=np.int64)
        _ck(_load().fhesi_ct_rot_sum_dev(self.h, _p(ka) if len(ka) else None, len(ka), logQ, base.ptr if base is not None else None, pre.ptr, count, nlimbs, out.ptr))

    def ct_matvec_bsgs_dev(self, baby_hoisted, kb, giant_hoisted, kg, nk: int, plain: "Plain", logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf,
                           decomp_bytes: int = 3):
        """out[i] = Reduce(sum_g rot_kg[g](sum_j rot_kb[j](src[i]) (*) plain[g B + j])), B = len(kb), G = len(kg), (G - 1) B < nk <= G B: the words of
        ct_rotations_dev for the babies, ct_plain_sum_dev with G groups per ciphertext, ct_rotations_dev per giant and ct_add_dev.  plain[g B + j] holds
        the diagonal g B + j rotated back by the giant step g (SlotSpace.bsgs_diagonals)."""
        hb, ka = self._hoisted_args(baby_hoisted, kb)
        hg, kc = self._hoisted_args(giant_hoisted, kg)
        _ck(_load().fhesi_ct_matvec_bsgs_dev(self.h, hb, _p(ka), len(ka), hg, _p(kc), len(kc), nk, plain.h, logQ, decomp_bytes, src.ptr, nlimbs, count, out.ptr))

    # ---- folds (fhesi_ct_rot_fold_dev): y <- y + rot_k(y) over a list of k, SumBatchedData on hoisted matrices
    def ct_rot_fold_dev(self, hoisted, ks, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """y_0 = Reduce(src), y_{s+1} = Reduce(y_s + rot_ks[s](y_s)), out = the last y: per step the words of ct_rotations_dev with one matrix followed
        by ct_add_dev.  hoisted[s]: the hoisted matrix of ks[s], or None with ks[s] = 1.  out may be src."""
        hs, ka = self._hoisted_args(hoisted, ks)
        _ck(_load().fhesi_ct_rot_fold_dev(self.h, hs, _p(ka) if len(ka) else None, len(ka), logQ, decomp_bytes, src.ptr, nlimbs, count, out.ptr))

    # ---- polynomial activations: scalar linear combinations and y = f(x) slot by slot (fhesi_ct_lin_comb_dev, fhesi_ct_poly_eval_dev)
    def ct_lin_comb_dev(self, logQ: int, p: int, pool, npool: int, nlimbs: int, a_idx, coef, seg, konst, out: DevBuf):
        """out[g] = Reduce(sum_{t in [seg[g], seg[g+1])} coef[t] pool[a_idx[t]] + konst[g]) on unscaled two-part ciphertexts: the words of a copy,
        ct_mul_long_dev and ct_add_dev per term and ct_add_const_dev with (konst[g], 0, .., 0).  coef, konst: any int64; konst None: no constants.
        The arguments are checked by the library (FhesiError names what it refuses)."""
        ia, sg = np.ascontiguousarray(a_idx, dtype=np.int32), np.ascontiguousarray(seg, dtype=np.int32)
        cf = np.ascontiguousarray(coef, dtype=np.int64)
        kn = None if konst is None else np.ascontiguousarray(konst, dtype=np.int64)
        if len(ia) != len(cf) or (kn is not None and len(kn) != len(sg) - 1):
            raise ValueError("ct_lin_comb_dev: one coefficient per term and one constant per group")
        _ck(_load().fhesi_ct_lin_comb_dev(self.h, logQ, p, pool.ptr if pool is not None else None, npool, nlimbs, _p(ia) if len(ia) else None,
                                          _p(cf) if len(cf) else None, _p(sg), _p(kn) if kn is not None else None, len(sg) - 1, out.ptr))

    def ct_poly_eval_dev(self, ksk: "KeySwitchMatrix", logQ: int, p: int, coef, src: DevBuf, nlimbs: int, count: int, out: DevBuf, baby: int = 0, decomp_bytes: int = 3):
        """out[i] = f(src[i]) slot by slot, f = sum_k coef[k] X^k (any int64, reduced modulo p): Paterson-Stockmeyer with `baby` baby powers (0: the
        planner's, poly_eval_plan) -- word for word the composition of ct_mul_sum_relin_dev and ct_lin_comb_dev that tests/poly_model.py states."""
        cf = np.ascontiguousarray(coef, dtype=np.int64)
        if cf.ndim != 1 or len(cf) < 2:
            raise ValueError("ct_poly_eval_dev: coef is [degree + 1], degree >= 1")
        _ck(_load().fhesi_ct_poly_eval_dev(self.h, ksk.h, logQ, p, decomp_bytes, _p(cf), len(cf) - 1, int(baby), src.ptr, nlimbs, count, out.ptr))

    def release_host_staging(self):
        """hand back the pinned + device staging ring the host-buffer calls keep between uses"""
        _ck(_load().fhesi_host_stage_release(self.h))


def matvec_bsgs_plan(nk: int) -> tuple:
    """(B, G) for nk diagonals: the B that minimises (B - 1) + (G - 1) with G = ceil(nk / B), of equal sums the larger B.  Touches no device."""
    b, g = _i32(0), _i32(0)
    _ck(_load().fhesi_matvec_bsgs_plan(int(nk), C.byref(b), C.byref(g)))
    return b.value, g.value


def poly_eval_plan(degree: int, baby: int = 0) -> dict:
    """The Paterson-Stockmeyer plan of a dense polynomial of degree 1 .. 4096 (fhesi_poly_eval_plan): B baby powers (baby = 0: the B of least key
    switches, of equal ones the smaller depth, then the larger B), G = degree // B + 1 groups, the products, the key switches and the multiplicative
    depth of Context.ct_poly_eval_dev.  Raises FhesiError naming the condition on a refused shape.  Touches no device."""
    v = [_i32(0) for _ in range(5)]
    _ck(_load().fhesi_poly_eval_plan(int(degree), int(baby), *(_byref(x) for x in v)))
    return dict(zip(("B", "G", "nprod", "nks", "depth"), (x.value for x in v)))


def linear_plan(cols: int, R: int, C: int, baby: int = 0) -> dict:
    """The plan of an R x C layer on rows of `cols` slots (fhesi_linear_plan): T = min(R, C) diagonals in G giant steps of B baby steps (baby = 0:
    the B of matvec_bsgs_plan(T)), nfold = log2(C / R) folds for R < C, and the rotation amounts in the order Linear.apply takes their matrices --
    babies 1 .. B - 1, giants B .. (G - 1) B, folds C/2 .. R.  Raises FhesiError naming the condition on a refused shape.  Touches no device."""
    T, B, G, nfold = _i32(0), _i32(0), _i32(0), _i32(0)
    _ck(_load().fhesi_linear_plan(int(cols), int(R), int(C), int(baby), _byref(T), _byref(B), _byref(G), _byref(nfold), None))
    amounts = np.zeros(B.value - 1 + G.value - 1 + nfold.value, dtype=np.int64)
    _ck(_load().fhesi_linear_plan(int(cols), int(R), int(C), int(baby), None, None, None, None, _p(amounts) if len(amounts) else None))
    return {"T": T.value, "B": B.value, "G": G.value, "nfold": nfold.value, "amounts": [int(a) for a in amounts]}


def linear_grid_plan(cols: int, R: int, C: int, Rb: int, Cb: int, baby: int = 0) -> dict:
    """The plan of an R x C matrix as a grid of Rb x Cb blocks on rows of `cols` slots (fhesi_linear_grid_plan): nI x nJ blocks, the block's T and
    nfold, B (baby = 0: the B that minimises nJ (B - 1) + nI (G - 1), of equal costs the larger), G, and the amounts in linear_plan's order.
    "key_switches" is nJ (B - 1) + nI (G - 1) + nI nfold, what LinearGrid.apply runs per item.  Raises FhesiError naming the condition on a refused
    shape.  Touches no device."""
    nI, nJ, T, B, G, nfold = (_i32(0) for _ in range(6))
    args = (int(cols), int(R), int(C), int(Rb), int(Cb), int(baby))
    _ck(_load().fhesi_linear_grid_plan(*args, _byref(nI), _byref(nJ), _byref(T), _byref(B), _byref(G), _byref(nfold), None))
    amounts = np.zeros(B.value - 1 + G.value - 1 + nfold.value, dtype=np.int64)
    _ck(_load().fhesi_linear_grid_plan(*args, None, None, None, None, None, None, _p(amounts) if len(amounts) else None))
    return {"nI": nI.value, "nJ": nJ.value, "T": T.value, "B": B.value, "G": G.value, "nfold": nfold.value, "amounts": [int(a) for a in amounts],
            "key_switches": nJ.value * (B.value - 1) + nI.value * (G.value - 1) + nI.value * nfold.value}


def conv2d_plan(cols: int, H: int, W: int, Cin: int, Cout: int, kh: int, kw: int, ah: int, aw: int, form: int = 0) -> dict:
    """The plan of a kh x kw convolution anchored at (ah, aw) over H x W planes, Cin -> Cout channels, on rows of `cols` slots (fhesi_conv2d_plan):
    form (given 0: the form of fewer key switches, flat on a tie; 1 flat, 2 split), nh and the amounts in the order Conv2d.apply takes their matrices --
    flat: entry t = dy kw + dx; split: the kw babies, then the kh giants; amount 0 exactly at the anchor --, the key switches per item and `terms`, the
    longest plaintext sum.  Raises FhesiError naming the condition on a refused shape.  Touches no device."""
    args = tuple(int(v) for v in (cols, H, W, Cin, Cout, kh, kw, ah, aw, form))
    f, nh, ks, terms = _i32(0), _i32(0), _i64(0), _i64(0)
    _ck(_load().fhesi_conv2d_plan(*args, _byref(f), _byref(nh), _byref(ks), _byref(terms), None))
    amounts = np.zeros(nh.value, dtype=np.int64)
    _ck(_load().fhesi_conv2d_plan(*args, None, None, None, None, _p(amounts)))
    return {"form": f.value, "nh": nh.value, "key_switches": ks.value, "terms": terms.value, "amounts": [int(a) for a in amounts]}


def _geometry(step, stride, dilation):
    """(sy, sx, ty, tx, ey, ex) of step, stride, dilation, each a pair of integers"""
    out = []
    for name, v in (("step", step), ("stride", stride), ("dilation", dilation)):
        if len(tuple(v)) != 2:
            raise ValueError(f"{name} = (vertical, horizontal)")
        out += [int(v[0]), int(v[1])]
    return tuple(out)


def conv2d_lattice_plan(cols: int, H: int, W: int, Cin: int, Cout: int, kh: int, kw: int, ah: int, aw: int, step=(1, 1), stride=(1, 1), dilation=(1, 1),
                        form: int = 0) -> dict:
    """conv2d_plan on a plane that carries a lattice step (fhesi_conv2d_lattice_plan): logical pixel (a, b) at physical pixel (a sy, b sx), the kernel
    read with stride (ty, tx) and dilation (ey, ex) on the logical plane.  The amounts are those of the offsets stretched to physical pixels; "out_step"
    = (sy ty, sx tx) is the step the next layer takes.  With the defaults: conv2d_plan.  Raises FhesiError naming the condition.  Touches no device."""
    args = tuple(int(v) for v in (cols, H, W, Cin, Cout, kh, kw, ah, aw)) + _geometry(step, stride, dilation) + (int(form),)
    f, nh, ks, terms, oy, ox = _i32(0), _i32(0), _i64(0), _i64(0), _i64(0), _i64(0)
    _ck(_load().fhesi_conv2d_lattice_plan(*args, _byref(f), _byref(nh), _byref(ks), _byref(terms), _byref(oy), _byref(ox), None))
    amounts = np.zeros(nh.value, dtype=np.int64)
    _ck(_load().fhesi_conv2d_lattice_plan(*args, None, None, None, None, None, None, _p(amounts)))
    return {"form": f.value, "nh": nh.value, "key_switches": ks.value, "terms": terms.value, "amounts": [int(a) for a in amounts], "out_step": (oy.value, ox.value)}


def pool2d_plan(cols: int, H: int, W: int, kh: int, kw: int, sy: int = 1, sx: int = 1, form: int = 0) -> dict:
    """The plan of a sum pooling over non-overlapping windows of kh x kw logical pixels on H x W planes of step (sy, sx) (fhesi_pool2d_plan): form (given 0:
    the form of fewer key switches, form 1 on a tie; 1 hoisted sums, 2 doubling), the amounts in the order SlotSpace.pool2d takes their matrices -- "nhor"
    horizontal ones, then the vertical ones --, the key switches per ciphertext, the key-switch levels and "out_step" = (sy kh, sx kw).  Raises FhesiError
    naming the condition on a refused shape.  Touches no device."""
    args = tuple(int(v) for v in (cols, H, W, kh, kw, sy, sx, form))
    f, nh, nhor, ks, lv, oy, ox = _i32(0), _i32(0), _i32(0), _i64(0), _i32(0), _i64(0), _i64(0)
    _ck(_load().fhesi_pool2d_plan(*args, _byref(f), _byref(nh), _byref(nhor), _byref(ks), _byref(lv), _byref(oy), _byref(ox), None))
    amounts = np.zeros(nh.value, dtype=np.int64)
    _ck(_load().fhesi_pool2d_plan(*args, None, None, None, None, None, None, None, _p(amounts) if nh.value else None))
    return {"form": f.value, "nh": nh.value, "nhor": nhor.value, "key_switches": ks.value, "levels": lv.value, "amounts": [int(a) for a in amounts],
            "out_step": (oy.value, ox.value)}


def plain_sum_bits(m: int, logQ: int, maxabs: int, terms: int) -> float:
    """Bits the chain product must exceed for a sum of `terms` ciphertext x plaintext products on the ring m: log2 of twice
    terms * growth * phi(m) * 2^(logQ-1) * maxabs, growth = 1 (m a power of two), 2 (m = q^k, 2 q^k) or phi(m).  Touches no device."""
    bits = C.c_double(0.0)
    _ck(_load().fhesi_plain_sum_bits(int(m), int(logQ), int(maxabs), int(terms), C.byref(bits)))
    return bits.value


class Plain:
    """nw prepared plaintext operands of one context (fhesi_plain): evaluation form over the whole chain, resident in HBM; made by
    SlotSpace.plain / Context.plain_from_poly, read by any number of Context.ct_plain_sum_dev calls."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h
        nw, maxabs, p = _i64(0), _u64(0), _u64(0)
        _ck(_load().fhesi_plain_info(self.h, C.byref(nw), C.byref(maxabs), C.byref(p)))
        self.nw, self.maxabs, self.p = nw.value, maxabs.value, p.value

    def close(self):
        if getattr(self, "h", None):
            _load().fhesi_plain_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _hoisted_by_amount(hoisted_by_amount, amounts, anchored: bool = False):
    """a mapping amount -> hoisted matrix covering `amounts` (anchored: the non-zero ones, None at 0), or the list of matrices in their order ->
    (the pointer array of a run call, its length)"""
    if hasattr(hoisted_by_amount, "keys"):
        hs = [hoisted_by_amount[a] if a or not anchored else None for a in amounts]
    else:
        hs = list(hoisted_by_amount)
    return (_vp * max(len(hs), 1))(*[h.h if h is not None else None for h in hs]), len(hs)


class _Layer:
    """What Linear, LinearGrid and Conv2d share: the handle on its space, the run call (_apply) through _run, close through _free (names of the C symbols) and
    _anchored -- whether .amounts holds a 0, which takes no matrix."""
    _run = _free = None
    _anchored = False

    def __init__(self, space: "SlotSpace", h):
        self.space, self.ctx, self.h = space, space.ctx, h

    def _apply(self, hoisted_by_amount, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int):
        arr, nh = _hoisted_by_amount(hoisted_by_amount, self.amounts, self._anchored)
        _ck(getattr(_load(), self._run)(self.ctx.h, self.h, arr, nh, logQ, decomp_bytes, src.ptr, nlimbs, count, out.ptr))

    def close(self):
        if getattr(self, "h", None):
            getattr(_load(), self._free)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Linear(_Layer):
    """One R x C layer y = M x + b on a slot space (fhesi_linear): its T = min(R, C) prepared diagonals, its replicated bias and its plan, resident in
    HBM; made by SlotSpace.linear.  .amounts lists the rotation amounts whose hoisted matrices apply() takes: babies, giants, folds."""
    _run, _free = "fhesi_ct_linear_dev", "fhesi_linear_free"

    def apply(self, hoisted_by_amount, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """out[i] = the layer of src[i] (fhesi_ct_linear_dev): src holds x replicated with period C in every row (SlotSpace.replicate), out holds
        M x + b with period R.  hoisted_by_amount: a mapping amount -> hoisted matrix of SlotSpace.rotation_k(amount) covering .amounts, or the
        list of matrices in the order of .amounts.  The words of SlotSpace.matvec_bsgs, SlotSpace.fold and SlotSpace.ct_add_slots_dev in that order."""
        self._apply(hoisted_by_amount, logQ, src, nlimbs, count, out, decomp_bytes)

    def __init__(self, space: "SlotSpace", h):
        super().__init__(space, h)
        R, Cc, T, B, G, nfold, bias = _i64(0), _i64(0), _i32(0), _i32(0), _i32(0), _i32(0), _i32(0)
        _ck(_load().fhesi_linear_info(self.h, _byref(R), _byref(Cc), _byref(T), _byref(B), _byref(G), _byref(nfold), _byref(bias), None))
        self.R, self.C, self.T, self.B, self.G, self.nfold, self.has_bias = R.value, Cc.value, T.value, B.value, G.value, nfold.value, bool(bias.value)
        a = np.zeros(self.B - 1 + self.G - 1 + self.nfold, dtype=np.int64)
        _ck(_load().fhesi_linear_info(self.h, None, None, None, None, None, None, None, _p(a) if len(a) else None))
        self.amounts = [int(x) for x in a]


class LinearGrid(_Layer):
    """An R x C matrix larger than a row of slots as a grid of nI x nJ blocks of Rb x Cb (fhesi_linear_grid): the prepared diagonals of every block,
    the replicated biases and the plan, resident in HBM; made by SlotSpace.linear_grid.  .amounts lists the rotation amounts whose hoisted matrices
    apply() takes -- babies, giants, the block's folds; .key_switches is what apply() runs per item."""
    _run, _free = "fhesi_ct_linear_grid_dev", "fhesi_linear_grid_free"

    def apply(self, hoisted_by_amount, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """out[I][i] = block row I of the product for item i (fhesi_ct_linear_grid_dev): src [nJ][count] holds SlotSpace.replicate_blocks(x, Cb)
        encrypted, out [nI][count] holds (M x + b)[I Rb ..] with period Rb.  hoisted_by_amount as Linear.apply takes it.  The babies of an input
        block serve every output block; the giants and folds of an output block run once, behind the sum over the input blocks."""
        self._apply(hoisted_by_amount, logQ, src, nlimbs, count, out, decomp_bytes)

    def __init__(self, space: "SlotSpace", h):
        super().__init__(space, h)
        R, Cc, Rb, Cb = _i64(0), _i64(0), _i64(0), _i64(0)
        nI, nJ, T, B, G, nfold, bias = (_i32(0) for _ in range(7))
        _ck(_load().fhesi_linear_grid_info(self.h, _byref(R), _byref(Cc), _byref(Rb), _byref(Cb), _byref(nI), _byref(nJ), _byref(T), _byref(B), _byref(G),
                                           _byref(nfold), _byref(bias), None))
        self.R, self.C, self.Rb, self.Cb, self.nI, self.nJ = R.value, Cc.value, Rb.value, Cb.value, nI.value, nJ.value
        self.T, self.B, self.G, self.nfold, self.has_bias = T.value, B.value, G.value, nfold.value, bool(bias.value)
        a = np.zeros(self.B - 1 + self.G - 1 + self.nfold, dtype=np.int64)
        _ck(_load().fhesi_linear_grid_info(self.h, None, None, None, None, None, None, None, None, None, None, None, _p(a) if len(a) else None))
        self.amounts = [int(x) for x in a]
        self.key_switches = self.nJ * (self.B - 1) + self.nI * (self.G - 1) + self.nI * self.nfold


class Conv2d(_Layer):
    """A 2-D convolution K [Cout][Cin][kh][kw] over H x W planes on a slot space, one channel per ciphertext (fhesi_conv2d): its masked weight
    plaintexts, its biases and its plan, resident in HBM; made by SlotSpace.conv2d.  .amounts lists the rotation amounts whose hoisted matrices apply()
    takes -- flat: entry t = dy kw + dx; split: the kw babies, then the kh giants; 0 (no matrix) exactly at the anchor; .key_switches is what apply()
    runs per item.  .step, .stride, .dilation: the lattice it was made for (all (1, 1) without one); .out_step = step * stride is the step of its output
    planes, which the next layer takes as its own."""
    _run, _free, _anchored = "fhesi_ct_conv2d_dev", "fhesi_conv2d_free", True

    def apply(self, hoisted_by_amount, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """out[I][i] = output channel I of item i (fhesi_ct_conv2d_dev): src [Cin][count] holds the input channels (SlotSpace.pack_images encrypted),
        out [Cout][count] the convolution with zero padding plus b[I].  hoisted_by_amount: a mapping amount -> hoisted matrix of
        SlotSpace.rotation_k(amount) covering the non-zero .amounts, or the list of matrices in the order of .amounts with None at the anchor."""
        self._apply(hoisted_by_amount, logQ, src, nlimbs, count, out, decomp_bytes)

    def __init__(self, space: "SlotSpace", h):
        super().__init__(space, h)
        v = [_i64(0) for _ in range(8)]
        form, nh, ks, terms, bias = _i32(0), _i32(0), _i64(0), _i64(0), _i32(0)
        _ck(_load().fhesi_conv2d_info(self.h, *(_byref(x) for x in v), _byref(form), _byref(nh), _byref(ks), _byref(terms), _byref(bias), None))
        self.Cout, self.Cin, self.kh, self.kw, self.H, self.W, self.ah, self.aw = (x.value for x in v)
        self.shape, self.image, self.anchor = (self.Cout, self.Cin, self.kh, self.kw), (self.H, self.W), (self.ah, self.aw)
        self.form, self.nh, self.key_switches, self.terms, self.has_bias = form.value, nh.value, ks.value, terms.value, bool(bias.value)
        a = np.zeros(self.nh, dtype=np.int64)
        _ck(_load().fhesi_conv2d_info(self.h, *([None] * 13), _p(a)))
        self.amounts = [int(x) for x in a]
        g = [_i64(0) for _ in range(8)]
        _ck(_load().fhesi_conv2d_lattice_info(self.h, *(_byref(x) for x in g)))
        g = [x.value for x in g]
        self.step, self.stride, self.dilation, self.out_step = (g[0], g[1]), (g[2], g[3]), (g[4], g[5]), (g[6], g[7])


def slots_plan(m: int, p: int, generator: int) -> dict:
    """The host half of PlaintextSpace::Init (no device, no context): checks (m, p, g) and returns total / usable slots, rho0, the number of
    auxiliary primes and the exponents e_j; raises FhesiError naming the failed condition on a refused ring."""
    total, usable, rho0, naux = _i64(0), _i64(0), _u64(0), _i32(0)
    _ck(_load().fhesi_slots_plan(m, p, generator, C.byref(total), C.byref(usable), C.byref(rho0), C.byref(naux), None))
    e = np.zeros(total.value, dtype=np.int32)
    _ck(_load().fhesi_slots_plan(m, p, generator, None, None, None, None, _p(e)))
    return {"total": total.value, "usable": usable.value, "rho0": rho0.value, "aux_primes": naux.value, "exps": e}


def slots_plan_pow2(m: int, p: int, generator: int) -> dict:
    """The host half of the two-row space of a power-of-two ring (m = 2^k, k >= 3, p = 1 mod m, g = 3 or 5 mod 8): total slots, rows, cols, rho0,
    the path (0 direct transform, 1 / 2 chirp with one / two auxiliary primes) and the exponents e_s; raises FhesiError on a refused ring."""
    total, rows, cols, rho0, path = _i64(0), _i64(0), _i64(0), _u64(0), _i32(0)
    _ck(_load().fhesi_slots_plan_pow2(m, p, generator, C.byref(total), C.byref(rows), C.byref(cols), C.byref(rho0), C.byref(path), None))
    e = np.zeros(total.value, dtype=np.int32)
    _ck(_load().fhesi_slots_plan_pow2(m, p, generator, None, None, None, None, None, _p(e)))
    return {"total": total.value, "rows": rows.value, "cols": cols.value, "rho0": rho0.value, "path": path.value, "exps": e}


class SlotSpace:
    """One PlaintextSpace on a context's GPU (fhesi_slots_create): batched EmbedInSlots / DecodeSlots and the slot-valued Encrypt / Decrypt.
    SlotSpace.pow2(ctx, p, g) makes the two-row space of a power-of-two ring (fhesi_slots_create_pow2) with the same methods."""

    def __init__(self, ctx: "Context", p: int, generator: int, _two_rows: bool = False, _borrowed=None):
        h = _borrowed
        if h is None:
            h = _vp()
            _ck((_load().fhesi_slots_create_pow2 if _two_rows else _load().fhesi_slots_create)(ctx.h, p, generator, C.byref(h)))
        self._from_handle(ctx, p, generator, h, owned=_borrowed is None)

    def _from_handle(self, ctx: "Context", p: int, generator: int, h, owned: bool = True):
        """The record of the space behind handle h.  A borrowed space (owned=False: a channel of a SlotBasis) does not free its handle."""
        self.ctx, self.p, self.generator, self.h, self.owned = ctx, p, generator, h, owned
        total, usable, rho0, naux = _i64(0), _i64(0), _u64(0), _i32(0)
        _ck(_load().fhesi_slots_info(self.h, C.byref(total), C.byref(usable), C.byref(rho0), C.byref(naux)))
        self.total, self.usable, self.rho0, self.aux_primes = total.value, usable.value, rho0.value, naux.value
        self._shape()

    @classmethod
    def pow2(cls, ctx: "Context", p: int, generator: int) -> "SlotSpace":
        """The two-row space: slot r * cols + j sits on rho0^((-1)^r g^j mod m)."""
        return cls(ctx, p, generator, _two_rows=True)

    def _shape(self):
        rows, cols, path = _i64(0), _i64(0), _i32(0)
        _ck(_load().fhesi_slots_shape(self.h, C.byref(rows), C.byref(cols), C.byref(path)))
        self.rows, self.cols, self.path = rows.value, cols.value, path.value

    def set_path(self, path: int):
        """Two-row spaces: 0 = the direct transform, otherwise the chirp (the results do not change)."""
        _ck(_load().fhesi_slots_set_path(self.h, path))
        self._shape()

    def close(self):
        if getattr(self, "h", None) and self.owned:
            _load().fhesi_slots_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def exponents(self) -> np.ndarray:
        e = np.zeros(self.total, dtype=np.int32)
        _ck(_load().fhesi_slots_exponents(self.h, _p(e)))
        return e

    def embed(self, vals: np.ndarray, only_usable: bool = True) -> np.ndarray:
        """vals [count][nvals] -> message polynomials [count][phi(m)] (EmbedInSlots)."""
        vals = np.ascontiguousarray(np.atleast_2d(vals), dtype=np.int64)
        msg = np.zeros((vals.shape[0], self.ctx.phim), dtype=np.int64)
        _ck(_load().fhesi_slots_embed(self.h, _p(vals), vals.shape[1], int(only_usable), vals.shape[0], _p(msg)))
        return msg

    def decode(self, msg: np.ndarray, nvals: int = None, only_usable: bool = True) -> np.ndarray:
        """message polynomials [count][phi(m)] -> slot values [count][nvals] (DecodeSlots)."""
        msg = np.ascontiguousarray(np.atleast_2d(msg), dtype=np.int64)
        nvals = self.total if nvals is None else nvals
        vals = np.zeros((msg.shape[0], nvals), dtype=np.int64)
        _ck(_load().fhesi_slots_decode(self.h, _p(msg), msg.shape[0], nvals, int(only_usable), _p(vals)))
        return vals

    def embed_dev(self, vals: DevBuf, nvals: int, count: int, msg: DevBuf, only_usable: bool = True):
        _ck(_load().fhesi_slots_embed_dev(self.h, vals.ptr, nvals, int(only_usable), count, msg.ptr))

    def decode_dev(self, msg: DevBuf, count: int, nvals: int, vals: DevBuf, only_usable: bool = True):
        _ck(_load().fhesi_slots_decode_dev(self.h, msg.ptr, count, nvals, int(only_usable), vals.ptr))

    def encrypt_batch_seeded(self, pk0: "DoubleCRT", pk1: "DoubleCRT", logQ: int, seed: int, first_index: int, vals: np.ndarray, out: DevBuf, nlimbs: int,
                             only_usable: bool = True):
        """Plaintext(context, vals[i]) + Encrypt under (seed, first_index + i); the message polynomials stay in HBM."""
        vals = np.ascontiguousarray(np.atleast_2d(vals), dtype=np.int64)
        _ck(_load().fhesi_encrypt_slots_batch_seeded(self.ctx.h, self.h, pk0.h, pk1.h, logQ, seed, first_index, _p(vals), vals.shape[1], int(only_usable),
                                                     vals.shape[0], out.ptr, nlimbs))

    def decrypt_batch(self, sk1: "DoubleCRT", logQ: int, ct: DevBuf, nlimbs: int, count: int, nvals: int = None, only_usable: bool = True) -> np.ndarray:
        nvals = self.total if nvals is None else nvals
        vals = np.zeros((count, nvals), dtype=np.int64)
        _ck(_load().fhesi_decrypt_slots_batch(self.ctx.h, self.h, sk1.h, logQ, ct.ptr, nlimbs, count, nvals, int(only_usable), _p(vals)))
        return vals

    def noise_budget(self, sk1: "DoubleCRT", logQ: int, ct: DevBuf, nlimbs: int, count: int, maxres: bool = False):
        """Context.noise_budget with this space's p."""
        return self.ctx.noise_budget(sk1, logQ, self.p, ct, nlimbs, count, maxres)

    def encrypt_noise_batch_seeded(self, pk0: "DoubleCRT", pk1: "DoubleCRT", logQ: int, seed: int, first_index: int, count: int, out: DevBuf, nlimbs: int):
        """Regression::GenerateNoise for `count` masks (slot 0 zero, the others uniform from (seed, index))."""
        _ck(_load().fhesi_encrypt_noise_batch_seeded(self.ctx.h, self.h, pk0.h, pk1.h, logQ, seed, first_index, count, out.ptr, nlimbs))

    def plain(self, vals: np.ndarray, only_usable: bool = True) -> Plain:
        """vals [nw][nvals] slot values -> a prepared handle for Context.ct_plain_sum_dev (embedded and transformed on the device)."""
        vals = np.ascontiguousarray(np.atleast_2d(vals), dtype=np.int64)
        h = _vp()
        _ck(_load().fhesi_plain_create_slots(self.h, _p(vals), vals.shape[1], int(only_usable), vals.shape[0], C.byref(h)))
        return Plain(self.ctx, h)

    # ---- hoisted rotations in slot terms: an amount t is the automorphism k = g^t mod m, as `>>=` takes it (t slots to the left in every row);
    # "swap" is k = m - 1, the row swap of a two-row space
    def rotation_k(self, amount) -> int:
        if amount == "swap":
            if self.rows != 2:
                raise ValueError("only a two-row space swaps rows")
            return self.ctx.m - 1
        return pow(self.generator, int(amount), self.ctx.m)

    def rotations(self, hoisted, amounts, logQ: int, src: DevBuf, nlimbs_in: int, count: int, out: DevBuf, nlimbs: int, decomp_bytes: int = 3):
        """Context.ct_rotations_dev with k = rotation_k(amount): hoisted[t] is the matrix of that k, hoisted (KeySwitchMatrix.hoist), or None for
        an amount whose k is 1 (no rotation).  out [len(amounts)][count] ciphertexts."""
        self.ctx.ct_rotations_dev(hoisted, [self.rotation_k(a) for a in amounts], logQ, src, nlimbs_in, count, out, nlimbs, decomp_bytes)

    def matvec(self, hoisted, amounts, plain: Plain, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """out[i] = sum_t rotate(src[i], amounts[t]) o plain[t] (Context.ct_matvec_dev): a matrix-vector product by diagonals, plain from
        SlotSpace.plain with diagonal t in row t."""
        self.ctx.ct_matvec_dev(hoisted, [self.rotation_k(a) for a in amounts], plain, logQ, src, nlimbs, count, out, decomp_bytes)

    # ---- baby-step/giant-step products: diagonal g B + j meets the baby rotation j inside the giant rotation g B, so it is rotated back by g B in the clear
    def rotate_values(self, vals: np.ndarray, amount: int) -> np.ndarray:
        """vals [..][total] slot values moved `amount` slots to the left in every row (negative: to the right): what `>>= g^amount` does to a plaintext."""
        v = np.asarray(vals)
        if v.shape[-1] != self.total:
            raise ValueError(f"rotate_values: {v.shape[-1]} values per plaintext, the space has {self.total} slots")
        rows = self.rows if self.rows == 2 else 1
        shaped = v.reshape(v.shape[:-1] + (rows, self.total // rows))
        return np.roll(shaped, -int(amount), axis=-1).reshape(v.shape)

    def bsgs_diagonals(self, diags: np.ndarray, B: int) -> np.ndarray:
        """diags [T][total] -> the operands of matvec_bsgs: row g B + j is rotate_values(diags[g B + j], -g B)."""
        d = np.asarray(diags)
        return np.stack([self.rotate_values(d[t], -(t // B) * B) for t in range(d.shape[0])])

    def matvec_bsgs(self, baby, giant, B: int, plain: Plain, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """out[i] = sum_t rotate(src[i], t) o d_t for t < plain.nw (Context.ct_matvec_bsgs_dev): baby[j] the hoisted matrix of g^j (j < B; None at j = 0),
        giant[i] that of g^(i B) (None at i = 0), plain = self.plain(self.bsgs_diagonals(d, B))."""
        nk = plain.nw
        G = (nk + B - 1) // B
        if len(baby) != B or len(giant) != G:
            raise ValueError(f"matvec_bsgs: {nk} diagonals in steps of {B} take {B} baby and {G} giant matrices, got {len(baby)} and {len(giant)}")
        self.ctx.ct_matvec_bsgs_dev(baby, [self.rotation_k(j) for j in range(B)], giant, [self.rotation_k(i * B) for i in range(G)], nk, plain, logQ, src, nlimbs,
                                    count, out, decomp_bytes)

    def ct_add_slots_dev(self, logQ: int, ct: DevBuf, nparts: int, nlimbs: int, count: int, vals: np.ndarray, only_usable: bool = True):
        """Ciphertext += Plaintext(vals) on unscaled ciphertexts; vals [nv][nvals] slot values, nv = 1 (one constant for all) or count."""
        vals = np.ascontiguousarray(np.atleast_2d(vals), dtype=np.int64)
        _ck(_load().fhesi_ct_add_slots_dev(self.ctx.h, self.h, logQ, ct.ptr, nparts, nlimbs, count, _p(vals), vals.shape[1], int(only_usable), vals.shape[0]))

    def poly_eval(self, ksk: "KeySwitchMatrix", coef, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, baby: int = 0, decomp_bytes: int = 3):
        """out[i] = f(src[i]) slot by slot modulo p, f = sum_k coef[k] X^k: the activation between two layers (Context.ct_poly_eval_dev with this
        space's p).  ksk: the s^2 -> s matrix."""
        self.ctx.ct_poly_eval_dev(ksk, logQ, self.p, coef, src, nlimbs, count, out, baby, decomp_bytes)

    # ---- dense linear layers: y = M x + b for a matrix given as a matrix (fhesi_linear_*): the diagonals are made on the device
    def fold(self, hoisted, amounts, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """y <- y + rotate(y, a) for a in amounts ("swap" included), out = the last y (Context.ct_rot_fold_dev with k = rotation_k(a)); out may be src.
        Over cols/2 .. 1 and "swap" it leaves the sum of all slots in every slot."""
        self.ctx.ct_rot_fold_dev(hoisted, [self.rotation_k(a) for a in amounts], logQ, src, nlimbs, count, out, decomp_bytes)

    def replicate(self, x, C: int) -> np.ndarray:
        """x [..][rows][C] (or [..][C] on a one-row space) -> slot values [..][total]: row r holds x_r with period C, the input layout of a layer with
        C columns.  C must divide the row.  Host only."""
        rows, cols = max(self.rows, 1), self.total // max(self.rows, 1)
        if C < 1 or cols % C:
            raise ValueError(f"replicate: period {C} does not divide the row of {cols} slots")
        x = np.asarray(x)
        lead = x.shape[:-2] if rows == 2 else x.shape[:-1]
        if x.shape[len(lead):] not in ((rows, C), (C,) if rows == 1 else None):
            raise ValueError(f"replicate: values of shape {x.shape}, a plaintext takes [{rows}][{C}]")
        v = x.reshape(lead + (rows, C))
        return np.ascontiguousarray(np.tile(v, cols // C).reshape(lead + (self.total,)))

    @staticmethod
    def _device_words(a, what: str):
        """a tensor in HBM (anything with data_ptr(), shape, and int64 elements: a torch tensor) -> (address, shape)"""
        if not hasattr(a, "data_ptr") or "int64" not in str(getattr(a, "dtype", "")) or not a.is_contiguous():
            raise ValueError(f"linear: device=True takes {what} as a contiguous int64 tensor in HBM")
        return _vp(a.data_ptr()), tuple(a.shape)

    def _tensor_args(self, who: str, T, bias, device: bool, name: str, dims, per: str):
        """a layer's tensor `name` with the dimensions named in `dims`, on the host or (device) in HBM, and its bias, one word per `per`, or None ->
        (pointer, bias pointer or None, shape, what the pointers keep alive)"""
        if device:
            tp, shape = self._device_words(T, f"the {name}")
        else:
            T = np.ascontiguousarray(T, dtype=np.int64)
            tp, shape = _p(T), T.shape
        if len(shape) != len(dims):
            raise ValueError(f"{who}: the {name} is " + "".join(f"[{d}]" for d in dims))
        bp = None
        if bias is not None:
            if device:
                bp, bshape = self._device_words(bias, "the bias")
            else:
                bias = np.ascontiguousarray(bias, dtype=np.int64)
                bp, bshape = _p(bias), bias.shape
            if bshape != (shape[0],):
                raise ValueError(f"{who}: a bias of shape {bshape} for {shape[0]} {per}")
        return tp, bp, shape, (T, bias)

    def _linear(self, who: str, create, layer, M, bias, block, baby: int, device: bool):
        """SlotSpace.linear (block None) and SlotSpace.linear_grid through `create`, the C constructor the method names"""
        tp, bp, (R, Cc), keep = self._tensor_args(who, M, bias, device, "matrix", ("R", "C"), "rows")
        h = _vp()
        _ck(create(self.h, tp, R, Cc, *(block(R, Cc) if block else ()), bp, int(baby), _byref(h)))
        return layer(self, h)

    def linear(self, M, bias=None, baby: int = 0, device: bool = False) -> Linear:
        """The layer y = M x + b for M [R][C], bias [R] or None, any int64 (reduced modulo p on the device).  device=True: M and bias are int64 tensors
        in HBM (torch tensors), read where they are.  baby: the baby step, 0 for the planner's.  Admitted shapes: linear_plan."""
        return self._linear("linear", _load().fhesi_linear_create_dev if device else _load().fhesi_linear_create, Linear, M, bias, None, baby, device)

    def linear_diagonals(self, M, baby: int = 0) -> np.ndarray:
        """The prepared slot vectors of the layer M [R][C]: [T][total], row g B + j the diagonal g B + j rotated back by g B (fhesi_linear_diagonals) --
        what SlotSpace.linear embeds, downloaded."""
        M = np.ascontiguousarray(M, dtype=np.int64)
        if M.ndim != 2:
            raise ValueError("linear_diagonals: the matrix is [R][C]")
        plan = linear_plan(self.total // max(self.rows, 1), M.shape[0], M.shape[1], baby)
        vals = np.zeros((plan["T"], self.total), dtype=np.int64)
        _ck(_load().fhesi_linear_diagonals(self.h, _p(M), M.shape[0], M.shape[1], int(baby), _p(vals)))
        return vals

    # ---- matrices larger than a row of slots: a grid of blocks (fhesi_linear_grid_*)
    def _grid_block(self, R: int, C: int, block):
        cols = self.total // max(self.rows, 1)
        return (min(R, cols), min(C, cols)) if block is None else (int(block[0]), int(block[1]))

    def linear_grid(self, M, bias=None, block=None, baby: int = 0, device: bool = False) -> LinearGrid:
        """The product y = M x + b for M [R][C] as a grid of blocks [Rb][Cb] = block (default (min(R, cols), min(C, cols))): R a multiple of Rb, C of
        Cb -- pad with zeros --, the block a shape linear_plan admits.  M, bias, device and baby as SlotSpace.linear takes them."""
        create = _load().fhesi_linear_grid_create_dev if device else _load().fhesi_linear_grid_create
        return self._linear("linear_grid", create, LinearGrid, M, bias, lambda R, Cc: self._grid_block(R, Cc, block), baby, device)

    def linear_grid_diagonals(self, M, block=None, baby: int = 0) -> np.ndarray:
        """The prepared slot vectors of the grid: [nI][nJ][T][total], entry (I, J) what linear_diagonals gives for the block M[I Rb .., J Cb ..] with
        the grid's B (fhesi_linear_grid_diagonals) -- what SlotSpace.linear_grid embeds, downloaded."""
        M = np.ascontiguousarray(M, dtype=np.int64)
        if M.ndim != 2:
            raise ValueError("linear_grid_diagonals: the matrix is [R][C]")
        Rb, Cb = self._grid_block(M.shape[0], M.shape[1], block)
        plan = linear_grid_plan(self.total // max(self.rows, 1), M.shape[0], M.shape[1], Rb, Cb, baby)
        vals = np.zeros((plan["nI"], plan["nJ"], plan["T"], self.total), dtype=np.int64)
        _ck(_load().fhesi_linear_grid_diagonals(self.h, _p(M), M.shape[0], M.shape[1], Rb, Cb, int(baby), _p(vals)))
        return vals

    # ---- convolution layers: image planes in the slots, one channel per ciphertext (fhesi_conv2d_*)
    @staticmethod
    def _conv_anchor(kh: int, kw: int, anchor):
        return ((kh - 1) // 2, (kw - 1) // 2) if anchor is None else (int(anchor[0]), int(anchor[1]))

    def conv2d(self, K, bias=None, image=None, anchor=None, form: int = 0, device: bool = False, step=(1, 1), stride=(1, 1), dilation=(1, 1)) -> Conv2d:
        """The convolution of K [Cout][Cin][kh][kw], bias [Cout] or None, any int64 (reduced modulo p on the device), over planes image = (H, W), H W
        dividing the row; zero padding, anchor (default ((kh - 1) // 2, (kw - 1) // 2)) the kernel entry that meets the output pixel.
        form: 0 the planner's, 1 flat, 2 split (conv2d_plan).  device=True: K and bias are int64 tensors in HBM (torch tensors), read where they are.
        step, stride, dilation: the lattice (conv2d_lattice_plan) -- the input's live pixels on every step-th row and column, the output's on every
        (step * stride)-th, every other output slot 0; all (1, 1), the default, goes through fhesi_conv2d_create."""
        if image is None:
            raise ValueError("conv2d: image = (H, W)")
        H, W = int(image[0]), int(image[1])
        kp, bp, shape, keep = self._tensor_args("conv2d", K, bias, device, "kernel", ("Cout", "Cin", "kh", "kw"), "output channels")
        ah, aw = self._conv_anchor(shape[2], shape[3], anchor)
        geom = _geometry(step, stride, dilation)
        h = _vp()
        if geom == (1,) * 6:
            create = _load().fhesi_conv2d_create_dev if device else _load().fhesi_conv2d_create
            _ck(create(self.h, kp, *shape, H, W, ah, aw, bp, int(form), _byref(h)))
        else:
            create = _load().fhesi_conv2d_lattice_create_dev if device else _load().fhesi_conv2d_lattice_create
            _ck(create(self.h, kp, *shape, H, W, ah, aw, *geom, bp, int(form), _byref(h)))
        return Conv2d(self, h)

    def _conv_masks(self, who: str, K, image, anchor, form: int, geom, lattice: bool):
        """conv2d_masks (a unit geometry: the entries without one) and conv2d_lattice_masks"""
        K = np.ascontiguousarray(K, dtype=np.int64)
        if K.ndim != 4:
            raise ValueError(f"{who}: the kernel is [Cout][Cin][kh][kw]")
        Cout, Cin, kh, kw = K.shape
        ah, aw = self._conv_anchor(kh, kw, anchor)
        lattice = lattice or _geometry(*geom) != (1,) * 6
        plan = conv2d_lattice_plan if lattice else conv2d_plan      # the shape, before the output is sized
        plan(self.total // max(self.rows, 1), image[0], image[1], Cin, Cout, kh, kw, ah, aw, *(geom if lattice else ()), form)
        vals = np.zeros((Cout, Cin, kh * kw, self.total), dtype=np.int64)
        args = (self.h, _p(K), Cout, Cin, kh, kw, int(image[0]), int(image[1]), ah, aw)
        if lattice:
            _ck(_load().fhesi_conv2d_lattice_masks(*args, *_geometry(*geom), int(form), _p(vals)))
        else:
            _ck(_load().fhesi_conv2d_masks(*args, int(form), _p(vals)))
        return vals

    def conv2d_masks(self, K, image, anchor=None, form: int = 0, step=(1, 1), stride=(1, 1), dilation=(1, 1)) -> np.ndarray:
        """The masked weight plaintexts of the convolution as slot values: [Cout][Cin][kh kw][total], entry t = dy kw + dx the weight under its mask,
        moved back by its giant amount in the split form (fhesi_conv2d_masks; with a step, stride or dilation other than (1, 1)
        fhesi_conv2d_lattice_masks) -- what SlotSpace.conv2d embeds, downloaded."""
        return self._conv_masks("conv2d_masks", K, image, anchor, form, (step, stride, dilation), False)

    def conv2d_lattice_masks(self, K, image, anchor=None, form: int = 0, step=(1, 1), stride=(1, 1), dilation=(1, 1)) -> np.ndarray:
        """conv2d_masks through fhesi_conv2d_lattice_masks whatever the geometry: with all (1, 1) the words of conv2d_masks, through the other entry."""
        return self._conv_masks("conv2d_lattice_masks", K, image, anchor, form, (step, stride, dilation), True)

    # ---- sum pooling and the bridge to a dense layer on a lattice of the plane (fhesi_ct_pool2d_dev, fhesi_slots_lattice_columns)
    def pool2d(self, hoisted_by_amount, image, window, step, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, form: int = 0, decomp_bytes: int = 3) -> dict:
        """out[i] = the sums of src[i] over non-overlapping windows = (kh, kw) of logical pixels on planes image = (H, W) of step = (sy, sx), each at its
        window's top left pixel (fhesi_ct_pool2d_dev): rotations and sums only, no plaintext product.  A SUM -- fold 1 / (kh kw) into the next layer.
        count: channels and items alike.  hoisted_by_amount: a mapping amount -> hoisted matrix of rotation_k(amount) covering pool2d_plan's amounts, or
        the list of matrices in their order.  out may be src.  Returns the plan; its "out_step" is the step of the result."""
        H, W, kh, kw, sy, sx = (int(v) for v in (image[0], image[1], window[0], window[1], step[0], step[1]))
        pl = pool2d_plan(self.total // max(self.rows, 1), H, W, kh, kw, sy, sx, form)
        arr, nh = _hoisted_by_amount(hoisted_by_amount, pl["amounts"])
        _ck(_load().fhesi_ct_pool2d_dev(self.h, H, W, kh, kw, sy, sx, int(form), arr, nh, logQ, decomp_bytes, src.ptr, nlimbs, count, out.ptr))
        return pl

    def lattice_columns(self, M, nch: int, image, step, device: bool = False, out=None):
        """M [R][nch Hl Wl] over the logical pixels of nch planes image = (H, W) of step = (sy, sx) -> M' [R][nch H W] over their slots, zero columns off
        the lattice (fhesi_slots_lattice_columns): what linear_grid(M', block=(Rb, H W)) takes as it is.  device=True: M and `out` are contiguous int64
        tensors in HBM (torch tensors); out is filled and returned."""
        H, W, sy, sx = (int(v) for v in (image[0], image[1], step[0], step[1]))
        if device:
            mp, shape = self._device_words(M, "the matrix")
            if out is None:
                raise ValueError("lattice_columns: device=True fills `out`, an int64 tensor [R][nch H W] in HBM")
            op, oshape = self._device_words(out, "the output")
            if len(shape) != 2 or oshape != (shape[0], int(nch) * H * W):
                raise ValueError(f"lattice_columns: a matrix of shape {shape} into an output of shape {oshape}")
            if sy < 1 or sx < 1 or H % sy or W % sx or shape[1] != int(nch) * (H // sy) * (W // sx):
                raise ValueError(f"lattice_columns: {shape[1]} columns are not {nch} logical planes of {H} x {W} at step ({sy}, {sx})")
            _ck(_load().fhesi_slots_lattice_columns_dev(self.h, mp, shape[0], int(nch), H, W, sy, sx, op))
            return out
        M = np.ascontiguousarray(M, dtype=np.int64)
        if M.ndim != 2 or sy < 1 or sx < 1 or H < 1 or W < 1 or H % sy or W % sx or M.shape[1] != int(nch) * (H // sy) * (W // sx):
            raise ValueError(f"lattice_columns: a matrix of shape {M.shape} is not [R][{nch} logical planes of {H} x {W} at step ({sy}, {sx})]")
        res = np.zeros((M.shape[0], int(nch) * H * W), dtype=np.int64)
        _ck(_load().fhesi_slots_lattice_columns(self.h, _p(M), M.shape[0], int(nch), H, W, sy, sx, _p(res)))
        return res

    def pack_images(self, x, step=(1, 1)) -> np.ndarray:
        """x [..][rows][cols / P][H][W] (the rows axis dropped on a one-row space) -> slot values [..][total]: image (r, b) in the P-block b of row r,
        pixel (y, x) at y W + x.  step = (sy, sx): x holds the LOGICAL planes [Hl][Wl], pixel (a, b) goes to (a sy, b sx) of the H x W = Hl sy x Wl sx
        plane and the slots off the lattice are 0.  Host only."""
        x = np.asarray(x)
        if tuple(step) != (1, 1):
            sy, sx = int(step[0]), int(step[1])
            if sy < 1 or sx < 1 or x.ndim < 2:
                raise ValueError(f"pack_images: step ({sy}, {sx})")
            full = np.zeros(x.shape[:-2] + (x.shape[-2] * sy, x.shape[-1] * sx), dtype=x.dtype)
            full[..., ::sy, ::sx] = x
            x = full
        rows, cols = max(self.rows, 1), self.total // max(self.rows, 1)
        H, W = x.shape[-2:]
        lead = x.shape[:-4] if rows == 2 else x.shape[:-3]
        if H * W < 1 or cols % (H * W) or x.shape[len(lead):] != ((rows,) if rows == 2 else ()) + (cols // (H * W), H, W):
            raise ValueError(f"pack_images: images of shape {x.shape}, a plaintext takes [{rows}][cols / (H W)][H][W] on rows of {cols} slots")
        return np.ascontiguousarray(x.reshape(lead + (self.total,)))

    def unpack_images(self, vals, H: int, W: int, step=(1, 1)) -> np.ndarray:
        """The inverse: slot values [..][total] -> [..][rows][cols / P][H][W] (the rows axis dropped on a one-row space); step = (sy, sx): only the
        lattice's pixels, [..][H / sy][W / sx].  Host only."""
        if tuple(step) != (1, 1):
            sy, sx = int(step[0]), int(step[1])
            if sy < 1 or sx < 1 or H % sy or W % sx:
                raise ValueError(f"unpack_images: the step ({sy}, {sx}) does not divide the {H} x {W} plane")
            return self.unpack_images(vals, H, W)[..., ::sy, ::sx]
        vals = np.asarray(vals)
        rows, cols = max(self.rows, 1), self.total // max(self.rows, 1)
        if H < 1 or W < 1 or cols % (H * W) or vals.shape[-1] != self.total:
            raise ValueError(f"unpack_images: {vals.shape[-1] if vals.ndim else 0} values as {H} x {W} planes on rows of {cols} slots")
        return vals.reshape(vals.shape[:-1] + ((rows,) if rows == 2 else ()) + (cols // (H * W), H, W))

    def replicate_blocks(self, x, Cb: int) -> np.ndarray:
        """x [count][rows][C] (or [count][C] on a one-row space), C = nJ Cb -> slot values [nJ][count][total]: plaintext (J, i) holds x_i[J Cb ..
        (J + 1) Cb) with period Cb in every row, the input layout of LinearGrid.apply.  Host only."""
        x = np.asarray(x)
        C = x.shape[-1]
        if Cb < 1 or C % Cb:
            raise ValueError(f"replicate_blocks: {C} values per row are not a multiple of the block's {Cb} columns")
        return np.ascontiguousarray(np.stack([self.replicate(x[..., J * Cb:(J + 1) * Cb], Cb) for J in range(C // Cb)]))

    def collect_blocks(self, y, Rb: int) -> np.ndarray:
        """The inverse on the output side: decrypted slot values y [nI][count][total], block I with period Rb -> [count][rows][nI Rb] (the rows axis
        dropped on a one-row space): the first period of every row, the blocks side by side.  Host only."""
        y = np.asarray(y)
        rows, cols = max(self.rows, 1), self.total // max(self.rows, 1)
        if Rb < 1 or cols % Rb or y.ndim != 3 or y.shape[-1] != self.total:
            raise ValueError(f"collect_blocks: values of shape {y.shape} with period {Rb} on rows of {cols} slots")
        first = y.reshape(y.shape[0], y.shape[1], rows, cols)[..., :Rb]                 # [nI][count][rows][Rb]
        out = np.moveaxis(first, 0, 2).reshape(y.shape[1], rows, y.shape[0] * Rb)       # [count][rows][nI][Rb] -> [count][rows][R]
        return np.ascontiguousarray(out if self.rows == 2 else out[:, 0, :])


def slots_basis_plan(m: int, bits: int, prime_bits: int, generator: int) -> dict:
    """A slot basis for results of up to `bits` bits (host only): the largest primes = 1 mod m below 2^prime_bits, descending, until their
    product exceeds 2^(bits + 1); raises FhesiError naming the condition when there are too few or more than 32 would be needed."""
    k, limbs = _i32(0), _i32(0)
    primes = np.zeros(32, dtype=np.uint64)
    _ck(_load().fhesi_slots_basis_plan(m, bits, prime_bits, generator, C.byref(k), _p(primes), C.byref(limbs)))
    return {"primes": [int(x) for x in primes[:k.value]], "limbs": limbs.value}


def slots_basis_check(m: int, primes, generator: int) -> dict:
    """The host half of SlotBasis (no device, no context): the checks of the constructor; returns the limbs of a result and the modulus P."""
    pr = np.ascontiguousarray(list(primes), dtype=np.uint64)
    limbs, mod = _i32(0), np.zeros(16, dtype=np.uint64)
    _ck(_load().fhesi_slots_basis_check(m, _p(pr) if len(pr) else None, len(pr), generator, C.byref(limbs), _p(mod)))
    return {"limbs": limbs.value, "modulus": sum(int(x) << (64 * i) for i, x in enumerate(mod))}


def pack_limbs(vals, limbs: int = None) -> np.ndarray:
    """Integers (Python ints of any size, nested lists or an integer array) -> [...][L] int64 little-endian two's complement limbs.
    L = `limbs`, or the least that holds every value."""
    a = np.asarray(vals)
    if a.dtype != object:
        a64 = np.ascontiguousarray(a, dtype=np.int64)
        if limbs in (None, 1):
            return a64.reshape(a64.shape + (1,))
        out = np.empty(a64.shape + (limbs,), dtype=np.int64)
        out[..., 0] = a64
        out[..., 1:] = (a64 >> 63)[..., None]
        return out
    flat = [int(v) for v in a.reshape(-1)]
    need = max([1] + [((v if v >= 0 else ~v).bit_length() + 1 + 63) // 64 for v in flat])
    L = need if limbs is None else limbs
    if L < need:
        raise ValueError(f"pack_limbs: {need} limbs needed, {L} given")
    mask = (1 << (64 * L)) - 1
    raw = b"".join((v & mask).to_bytes(8 * L, "little") for v in flat)
    return np.frombuffer(raw, dtype=np.int64).reshape(a.shape + (L,)).copy()


def _value_limbs(vals, limbs):
    """[count][nvals][L] limbs of what a SlotBasis call was given: a 3-d int64 array is limbs already, anything else is integers to pack"""
    if isinstance(vals, np.ndarray) and vals.ndim == 3 and vals.dtype == np.int64:
        return np.ascontiguousarray(vals)
    return pack_limbs(np.atleast_2d(vals if isinstance(vals, np.ndarray) else np.asarray(vals)), limbs)


def unpack_limbs(limbs: np.ndarray) -> np.ndarray:
    """[...][L] two's complement limbs -> object array [...] of Python ints."""
    limbs = np.ascontiguousarray(limbs, dtype=np.int64)
    L = limbs.shape[-1]
    raw = limbs.tobytes()
    out = np.empty(limbs.shape[:-1], dtype=object)
    flat = out.reshape(-1)
    for i in range(flat.shape[0]):
        flat[i] = int.from_bytes(raw[8 * L * i: 8 * L * (i + 1)], "little", signed=True)
    return out


class _View:
    """one channel's part of a [k][count] device buffer"""

    def __init__(self, buf, off: int):
        self.ptr = _vp(buf.ptr.value + off)


class SlotBasis:
    """Integer slots over k plaintext primes on a two-row ring (fhesi_slots_basis_create): a slot holds a signed integer of (-P/2, P/2),
    P the product of the primes; a logical plaintext / ciphertext is k channel plaintexts / ciphertexts on ONE context and key set, channel c
    an ordinary two-row space modulo primes[c].  The caller owes |result| < P/2."""

    def __init__(self, ctx: "Context", primes, generator: int):
        self.ctx, self.generator = ctx, generator
        self.h = _vp()
        pr = np.ascontiguousarray(list(primes), dtype=np.uint64)
        _ck(_load().fhesi_slots_basis_create(ctx.h, _p(pr) if len(pr) else None, len(pr), generator, C.byref(self.h)))
        k, limbs, total, rows, cols = _i32(0), _i32(0), _i64(0), _i64(0), _i64(0)
        _ck(_load().fhesi_slots_basis_info(self.h, C.byref(k), _p(pr), C.byref(limbs), C.byref(total), C.byref(rows), C.byref(cols)))
        self.k, self.limbs, self.total, self.rows, self.cols = k.value, limbs.value, total.value, rows.value, cols.value
        self.primes = [int(x) for x in pr]
        self.modulus = 1
        for x in self.primes:
            self.modulus *= x
        self._channels = {}

    @classmethod
    def pow2(cls, ctx: "Context", primes, generator: int) -> "SlotBasis":
        return cls(ctx, primes, generator)

    @classmethod
    def plan(cls, ctx: "Context", bits: int, prime_bits: int, generator: int) -> "SlotBasis":
        """The basis slots_basis_plan picks for results of up to `bits` bits."""
        return cls(ctx, slots_basis_plan(ctx.m, bits, prime_bits, generator)["primes"], generator)

    def close(self):
        if getattr(self, "h", None):
            for s in self._channels.values():
                s.h = None                       # the basis owns the channels' spaces
            _load().fhesi_slots_basis_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def channel(self, c: int) -> "SlotSpace":
        """Channel c as a SlotSpace (p = primes[c]) for every existing call; it lives as long as the basis."""
        if c not in self._channels:
            h = _vp()
            _ck(_load().fhesi_slots_basis_channel(self.h, c, C.byref(h)))
            s = SlotSpace(self.ctx, self.primes[c], self.generator, _borrowed=h)
            s._basis = self
            self._channels[c] = s
        return self._channels[c]

    def embed(self, vals, limbs: int = None) -> np.ndarray:
        """vals [count][nvals] (Python ints or an int64 array; a 3-d int64 array is taken as limbs [count][nvals][L]) -> message polynomials
        [k][count][phi(m)]."""
        v = _value_limbs(vals, limbs)
        count, nvals, L = v.shape
        msg = np.zeros((self.k, count, self.total), dtype=np.int64)
        _ck(_load().fhesi_slots_basis_embed(self.h, _p(v), L, nvals, count, _p(msg)))
        return msg

    def decode(self, msg: np.ndarray, nvals: int = None, raw: bool = False) -> np.ndarray:
        """message polynomials [k][count][phi(m)] -> [count][nvals] Python ints in (-P/2, P/2) (raw: the limbs [count][nvals][L])."""
        msg = np.ascontiguousarray(msg, dtype=np.int64)
        if msg.ndim == 2:
            msg = msg[:, None, :]
        nvals = self.total if nvals is None else nvals
        out = np.zeros((msg.shape[1], nvals, self.limbs), dtype=np.int64)
        _ck(_load().fhesi_slots_basis_decode(self.h, _p(msg), msg.shape[1], nvals, _p(out)))
        return out if raw else unpack_limbs(out)

    def embed_dev(self, vals: DevBuf, limbs: int, nvals: int, count: int, msg: DevBuf):
        _ck(_load().fhesi_slots_basis_embed_dev(self.h, vals.ptr, limbs, nvals, count, msg.ptr))

    def decode_dev(self, msg: DevBuf, count: int, nvals: int, vals: DevBuf):
        _ck(_load().fhesi_slots_basis_decode_dev(self.h, msg.ptr, count, nvals, vals.ptr))

    def encrypt_batch_seeded(self, pk0: "DoubleCRT", pk1: "DoubleCRT", logQ: int, seed: int, first_index: int, vals, out: DevBuf, nlimbs: int, limbs: int = None):
        """`count` logical plaintexts -> out [k][count] ciphertexts; channel c, plaintext i under (seed, first_index + c * count + i)."""
        v = _value_limbs(vals, limbs)
        count, nvals, L = v.shape
        _ck(_load().fhesi_encrypt_int_slots_batch_seeded(self.ctx.h, self.h, pk0.h, pk1.h, logQ, seed, first_index, _p(v), L, nvals, count, out.ptr, nlimbs))

    def decrypt_batch(self, sk1: "DoubleCRT", logQ: int, ct: DevBuf, nlimbs: int, count: int, nvals: int = None, raw: bool = False) -> np.ndarray:
        nvals = self.total if nvals is None else nvals
        out = np.zeros((count, nvals, self.limbs), dtype=np.int64)
        _ck(_load().fhesi_decrypt_int_slots_batch(self.ctx.h, self.h, sk1.h, logQ, ct.ptr, nlimbs, count, nvals, _p(out)))
        return out if raw else unpack_limbs(out)

    def noise_budget(self, sk1: "DoubleCRT", logQ: int, ct: DevBuf, nlimbs: int, count: int):
        """ct [k][count] -> (budgets [k][count] with p = primes[c] in channel c, their minimum over the channels [count])."""
        budget = np.zeros((self.k, count), dtype=np.int32)
        _ck(_load().fhesi_ct_noise_int_batch(self.ctx.h, self.h, sk1.h, logQ, ct.ptr, nlimbs, count, _p(budget)))
        return budget, budget.min(axis=0)

    # prepared plaintext operands, channel by channel (no entry point of their own: channel c is an ordinary space modulo primes[c])
    def _residues(self, vals, c: int) -> np.ndarray:
        """integers (Python ints of any size or an integer array) [..][nvals] -> their residues modulo primes[c], int64"""
        a = np.atleast_2d(np.asarray(vals))
        if a.dtype == object:
            return np.array([[int(v) % self.primes[c] for v in row] for row in a], dtype=np.int64)
        return np.mod(a.astype(np.int64), np.int64(self.primes[c]))

    def plain(self, vals) -> list:
        """vals [nw][nvals] integers -> the k channel handles (channel c holds vals mod primes[c])."""
        return [self.channel(c).plain(self._residues(vals, c)) for c in range(self.k)]

    def ct_plain_sum_dev(self, plains, logQ: int, pool: DevBuf, npool: int, nlimbs: int, a_idx, b_idx, seg, out: DevBuf):
        """Context.ct_plain_sum_dev per channel: pool [k][npool], out [k][ngroups] logical ciphertexts, plains from SlotBasis.plain."""
        words = 2 * self.ctx.phim * nlimbs * 8
        ngroups = len(seg) - 1
        for c in range(self.k):
            self.ctx.ct_plain_sum_dev(plains[c], logQ, _View(pool, c * npool * words), npool, nlimbs, a_idx, b_idx, seg, _View(out, c * ngroups * words))

    def rotations(self, hoisted, amounts, logQ: int, src: DevBuf, nlimbs_in: int, count: int, out: DevBuf, nlimbs: int, decomp_bytes: int = 3):
        """SlotSpace.rotations per channel (one key set serves every channel): src [k][count], out [k][len(amounts)][count] ciphertexts."""
        win, wout = 2 * self.ctx.phim * nlimbs_in * 8, 2 * self.ctx.phim * nlimbs * 8
        for c in range(self.k):
            self.channel(c).rotations(hoisted, amounts, logQ, _View(src, c * count * win), nlimbs_in, count, _View(out, c * len(amounts) * count * wout), nlimbs, decomp_bytes)

    def matvec(self, hoisted, amounts, plains, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """SlotSpace.matvec per channel: src, out [k][count] logical ciphertexts, plains from SlotBasis.plain (diagonal t in row t)."""
        words = 2 * self.ctx.phim * nlimbs * 8
        for c in range(self.k):
            self.channel(c).matvec(hoisted, amounts, plains[c], logQ, _View(src, c * count * words), nlimbs, count, _View(out, c * count * words), decomp_bytes)

    def matvec_bsgs(self, baby, giant, B: int, plains, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """SlotSpace.matvec_bsgs per channel: src, out [k][count] logical ciphertexts, plains = SlotBasis.plain of the diagonals that
        channel(0).bsgs_diagonals rotated back (the rotation moves slots, whatever the prime)."""
        words = 2 * self.ctx.phim * nlimbs * 8
        for c in range(self.k):
            self.channel(c).matvec_bsgs(baby, giant, B, plains[c], logQ, _View(src, c * count * words), nlimbs, count, _View(out, c * count * words), decomp_bytes)

    def linear(self, M, bias=None, baby: int = 0) -> list:
        """SlotSpace.linear per channel: the k handles of the layer M [R][C], bias [R] (integers of any size), channel c holding them modulo primes[c]."""
        return [self.channel(c).linear(self._residues(M, c), None if bias is None else self._residues(bias, c)[0], baby) for c in range(self.k)]

    def linear_apply(self, layers, hoisted_by_amount, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """Linear.apply per channel (one key set serves every channel): src, out [k][count] logical ciphertexts, layers from SlotBasis.linear."""
        words = 2 * self.ctx.phim * nlimbs * 8
        for c in range(self.k):
            layers[c].apply(hoisted_by_amount, logQ, _View(src, c * count * words), nlimbs, count, _View(out, c * count * words), decomp_bytes)

    def conv2d(self, K, bias=None, image=None, anchor=None, form: int = 0, step=(1, 1), stride=(1, 1), dilation=(1, 1)) -> list:
        """SlotSpace.conv2d per channel: the k handles of the convolution K [Cout][Cin][kh][kw], bias [Cout] (integers of any size), channel c holding
        them modulo primes[c]; step, stride, dilation as SlotSpace.conv2d takes them."""
        K = np.asarray(K)
        out = []
        for c in range(self.k):
            Kc = self._residues(K.reshape(1, -1), c).reshape(K.shape)
            out.append(self.channel(c).conv2d(Kc, None if bias is None else self._residues(bias, c)[0], image, anchor, form, step=step, stride=stride, dilation=dilation))
        return out

    def pool2d(self, hoisted_by_amount, image, window, step, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, form: int = 0, decomp_bytes: int = 3) -> dict:
        """SlotSpace.pool2d channel by channel (one key set serves every channel): src, out [k][count] logical ciphertexts.  Exact while the window sums
        stay below half the product of the primes."""
        words = 2 * self.ctx.phim * nlimbs * 8
        pl = None
        for c in range(self.k):
            pl = self.channel(c).pool2d(hoisted_by_amount, image, window, step, logQ, _View(src, c * count * words), nlimbs, count, _View(out, c * count * words), form, decomp_bytes)
        return pl

    def conv2d_apply(self, layers, hoisted_by_amount, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, decomp_bytes: int = 3):
        """Conv2d.apply per channel (one key set serves every channel): src [k][Cin][count], out [k][Cout][count] logical ciphertexts, layers from
        SlotBasis.conv2d."""
        words = 2 * self.ctx.phim * nlimbs * 8
        for c in range(self.k):
            layers[c].apply(hoisted_by_amount, logQ, _View(src, c * layers[c].Cin * count * words), nlimbs, count, _View(out, c * layers[c].Cout * count * words), decomp_bytes)

    def poly_eval(self, ksk: "KeySwitchMatrix", coef, logQ: int, src: DevBuf, nlimbs: int, count: int, out: DevBuf, baby: int = 0, decomp_bytes: int = 3):
        """SlotSpace.poly_eval per channel (one key set serves every channel): src, out [k][count] logical ciphertexts; coef Python integers of any
        size, channel c taking them modulo primes[c].  Exact while |f(v)| stays below half the product of the primes."""
        words = 2 * self.ctx.phim * nlimbs * 8
        for c in range(self.k):
            cf = [int(v) % self.primes[c] for v in coef]
            self.channel(c).poly_eval(ksk, cf, logQ, _View(src, c * count * words), nlimbs, count, _View(out, c * count * words), baby, decomp_bytes)

    def ct_add_slots_dev(self, logQ: int, ct: DevBuf, nlimbs: int, count: int, vals):
        """Ciphertext += integers, per channel: ct [k][count] two-part ciphertexts, vals [nv][nvals] integers, nv = 1 or count."""
        words = 2 * self.ctx.phim * nlimbs * 8
        for c in range(self.k):
            self.channel(c).ct_add_slots_dev(logQ, _View(ct, c * count * words), 2, nlimbs, count, self._residues(vals, c))

    def encrypt_noise_batch_seeded(self, pk0: "DoubleCRT", pk1: "DoubleCRT", logQ: int, seed: int, first_index: int, count: int, out: DevBuf, nlimbs: int):
        """k masks per logical mask (slot 0 = 0 modulo P, the others uniform), object indices first_index .. first_index + k * count - 1."""
        _ck(_load().fhesi_encrypt_noise_int_batch_seeded(self.ctx.h, self.h, pk0.h, pk1.h, logQ, seed, first_index, count, out.ptr, nlimbs))


class DoubleCRT:
    """One DoubleCRT object resident in HBM (DoubleCRT.h:83-365 through the C ABI)."""

    def __init__(self, ctx: Context, index_set=None):
        self.ctx = ctx
        self.h = _vp()
        if index_set is None:
            _ck(_load().fhesi_dcrt_alloc(ctx.h, None, 0, C.byref(self.h)))
        else:
            ia = np.array(list(index_set), dtype=np.int32)
            if len(ia) == 0:
                raise FhesiError("DoubleCRT: empty index set")
            _ck(_load().fhesi_dcrt_alloc(ctx.h, _p(ia), len(ia), C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _load().fhesi_dcrt_free(self.h)
                self.h = None
        except Exception:
            pass

    @classmethod
    def from_poly(cls, ctx: Context, limbs: np.ndarray, index_set=None) -> "DoubleCRT":
        d = cls(ctx, index_set)
        d.assign_poly(limbs)
        return d

    def index_set(self):
        n = _i32(0)
        buf = np.zeros(self.ctx.L, dtype=np.int32)
        _ck(_load().fhesi_dcrt_index_set(self.h, _p(buf), C.byref(n)))
        return [int(x) for x in buf[:n.value]]

    def assign_poly(self, limbs: np.ndarray):
        limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
        _ck(_load().fhesi_dcrt_from_poly(self.h, _p(limbs), limbs.shape[1], limbs.shape[0]))

    def assign(self, other: "DoubleCRT"):
        _ck(_load().fhesi_dcrt_copy(self.h, other.h))

    def copy(self) -> "DoubleCRT":
        d = DoubleCRT(self.ctx, self.index_set())
        d.assign(self)
        return d

    def to_poly(self, nlimbs: int, index_set=None, positive: bool = False) -> np.ndarray:
        out = np.zeros((self.ctx.phim, nlimbs), dtype=np.uint64)
        if index_set is None:
            _ck(_load().fhesi_dcrt_to_poly(self.h, None, 0, int(positive), _p(out), nlimbs))
        else:
            ia = np.array(list(index_set), dtype=np.int32)
            if len(ia) == 0:      # empty intersection -> zero polynomial (DoubleCRT.cpp:354-357)
                return out
            _ck(_load().fhesi_dcrt_to_poly(self.h, _p(ia), len(ia), int(positive), _p(out), nlimbs))
        return out

    def row(self, prime: int) -> np.ndarray:
        out = np.zeros(self.ctx.phim, dtype=np.uint64)
        _ck(_load().fhesi_dcrt_download_row(self.h, prime, _p(out)))
        return out

    def sample(self, kind: int, param: int, seed: int, index: int):
        """DoubleCRT::sampleHWt(param) (kind 0) / sampleGaussian() (kind 1) drawn on the device from (seed, index) -- philox.h."""
        _ck(_load().fhesi_dcrt_sample(self.h, kind, param, seed, index))
        return self

    def set_row(self, prime: int, row: np.ndarray):
        row = np.ascontiguousarray(row, dtype=np.uint64)
        _ck(_load().fhesi_dcrt_upload_row(self.h, prime, _p(row)))

    def rows(self) -> np.ndarray:
        return np.stack([self.row(i) for i in self.index_set()])

    def op(self, other: "DoubleCRT", op: int):
        _ck(_load().fhesi_dcrt_op(self.h, other.h, op))
        return self

    def op_scalar(self, num: int, op: int, nlimbs: int = 4):
        mod = 1 << (64 * nlimbs)
        v = num % mod
        s = np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(nlimbs)], dtype=np.uint64)
        _ck(_load().fhesi_dcrt_op_scalar(self.h, _p(s), nlimbs, op))
        return self

    def automorph(self, k: int):
        _ck(_load().fhesi_dcrt_automorph(self.h, k))
        return self

    def exp(self, e: int):
        """DoubleCRT::Exp (DoubleCRT.cpp:423-434): element-wise PowerMod."""
        _ck(_load().fhesi_dcrt_exp(self.h, e))
        return self

    def add_primes(self, idx):
        ia = np.array(list(idx), dtype=np.int32)
        _ck(_load().fhesi_dcrt_add_primes(self.h, _p(ia), len(ia)))

    def remove_primes(self, idx):
        ia = np.array(list(idx), dtype=np.int32)
        _ck(_load().fhesi_dcrt_remove_primes(self.h, _p(ia), len(ia)))

    def add_primes_and_scale(self, idx, p: int) -> float:
        """DoubleCRT::addPrimesAndScale (DoubleCRT.cpp:162-208); returns the logarithm of the scaling factor."""
        ia = np.array(list(idx), dtype=np.int32)
        lf = C.c_double(0.0)
        _ck(_load().fhesi_dcrt_add_primes_and_scale(self.h, _p(ia), len(ia), p, C.byref(lf)))
        return lf.value

    def scale_down_to_set(self, idx, p: int):
        """DoubleCRT::scaleDownToSet (DoubleCRT.cpp:518-558)."""
        ia = np.array(list(idx), dtype=np.int32)
        _ck(_load().fhesi_dcrt_scale_down_to_set(self.h, _p(ia), len(ia), p))

    def equals(self, other: "DoubleCRT") -> bool:
        eq = _i32(0)
        _ck(_load().fhesi_dcrt_equal(self.h, other.h, C.byref(eq)))
        return bool(eq.value)

    def from_scrt(self, coeff_rows: np.ndarray):
        coeff_rows = np.ascontiguousarray(coeff_rows, dtype=np.uint64)
        _ck(_load().fhesi_dcrt_from_scrt(self.h, _p(coeff_rows)))

    def to_scrt(self) -> np.ndarray:
        out = np.zeros((len(self.index_set()), self.ctx.phim), dtype=np.uint64)
        _ck(_load().fhesi_dcrt_to_scrt(self.h, _p(out)))
        return out


class SingleCRT:
    """One SingleCRT object resident in HBM (SingleCRT.h:41-175 through the C ABI): coefficient residues per prime."""

    def __init__(self, ctx: Context, index_set=None):
        self.ctx = ctx
        self.h = _vp()
        if index_set is None:
            _ck(_load().fhesi_scrt_alloc(ctx.h, None, 0, C.byref(self.h)))
        else:
            ia = np.array(list(index_set), dtype=np.int32)
            if len(ia) == 0:
                raise FhesiError("SingleCRT: empty index set")
            _ck(_load().fhesi_scrt_alloc(ctx.h, _p(ia), len(ia), C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _load().fhesi_dcrt_free(self.h)
                self.h = None
        except Exception:
            pass

    index_set = DoubleCRT.index_set
    row = DoubleCRT.row
    set_row = DoubleCRT.set_row
    rows = DoubleCRT.rows
    remove_primes = DoubleCRT.remove_primes

    def assign_poly(self, limbs: np.ndarray):
        limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
        _ck(_load().fhesi_scrt_from_poly(self.h, _p(limbs), limbs.shape[1], limbs.shape[0]))
        return self

    def to_poly(self, nlimbs: int, index_set=None) -> np.ndarray:
        out = np.zeros((self.ctx.phim, nlimbs), dtype=np.uint64)
        if index_set is None:
            _ck(_load().fhesi_scrt_to_poly(self.h, None, 0, _p(out), nlimbs))
        else:
            ia = np.array(list(index_set), dtype=np.int32)
            if len(ia) == 0:
                return out
            _ck(_load().fhesi_scrt_to_poly(self.h, _p(ia), len(ia), _p(out), nlimbs))
        return out

    def assign(self, other: "SingleCRT"):
        _ck(_load().fhesi_dcrt_copy(self.h, other.h))

    def op(self, other: "SingleCRT", op: int):
        _ck(_load().fhesi_dcrt_op(self.h, other.h, op))
        return self

    def op_scalar(self, num: int, op: int, nlimbs: int = 4):
        mod = 1 << (64 * nlimbs)
        v = num % mod
        s = np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(nlimbs)], dtype=np.uint64)
        _ck(_load().fhesi_scrt_op_scalar(self.h, _p(s), nlimbs, op))
        return self

    def equals(self, other) -> bool:
        eq = _i32(0)
        _ck(_load().fhesi_dcrt_equal(self.h, other.h, C.byref(eq)))
        return bool(eq.value)

    def assign_dcrt(self, d: DoubleCRT, index_set=None):
        """DoubleCRT::toSingleCRT (DoubleCRT.cpp:498-515)."""
        if index_set is None:
            _ck(_load().fhesi_scrt_assign_dcrt(self.h, d.h, None, 0))
        else:
            ia = np.array(list(index_set), dtype=np.int32)
            _ck(_load().fhesi_scrt_assign_dcrt(self.h, d.h, _p(ia), len(ia)))
        return self


def dcrt_assign_scrt(d: DoubleCRT, s: SingleCRT):
    """DoubleCRT::operator=(const SingleCRT&) (DoubleCRT.cpp:484-496)."""
    _ck(_load().fhesi_dcrt_assign_scrt(d.h, s.h))
    return d


class Comm:
    """One rank of a multi-GPU group (fhesi_comm: an RCCL communicator; a loopback group when ranks share a device).  Collective
    methods must be called by every rank of the group concurrently (one host thread per rank; ctypes releases the GIL)."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def init_all(devices):
        devs = np.array(list(devices), dtype=np.int32)
        hs = (_vp * len(devs))()
        _ck(_load().fhesi_comm_init_all(len(devs), _p(devs), hs))
        return [Comm(_vp(h)) for h in hs]

    @property
    def rank(self) -> int:
        return _load().fhesi_comm_rank(self.h)

    @property
    def size(self) -> int:
        return _load().fhesi_comm_size(self.h)

    def ksk_broadcast(self, ksk: "KeySwitchMatrix", root: int = 0):
        _ck(_load().fhesi_ksk_broadcast(ksk.h, self.h, root))

    def exchange(self, ctx: Context, base: DevBuf, offsets_words):
        off = np.ascontiguousarray(offsets_words, dtype=np.int64)
        _ck(_load().fhesi_comm_exchange(ctx.h, self.h, base.ptr, _p(off)))

    def exchange_begin(self, ctx: Context, base: DevBuf, offsets_words):
        """the exchange enqueued on the communicator's own stream behind the context's stream; returns without waiting for the GPU"""
        off = np.ascontiguousarray(offsets_words, dtype=np.int64)
        _ck(_load().fhesi_comm_exchange_begin(ctx.h, self.h, base.ptr, _p(off)))

    def exchange_end(self, ctx: Context):
        """every exchange begun since the last end has landed"""
        _ck(_load().fhesi_comm_exchange_end(ctx.h, self.h))

    def allreduce_rows(self, ctx: Context, rows: DevBuf, count: int):
        _ck(_load().fhesi_comm_allreduce_rows(ctx.h, self.h, rows.ptr, count))

    def destroy(self):
        if self.h:
            _load().fhesi_comm_destroy(self.h)
            self.h = None


class KeySwitchMatrix:
    """KeySwitchSI::keySwitchMatrix resident in HBM: [2][ncomp*ndigits][L][phim]."""

    def __init__(self, ctx: Context, ncomp: int, ndigits: int):
        self.ctx, self.ncomp, self.ndigits = ctx, ncomp, ndigits
        self.h = _vp()
        _ck(_load().fhesi_ksk_create(ctx.h, ncomp, ndigits, C.byref(self.h)))

    def upload(self, rows: np.ndarray):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        assert rows.nbytes == self.nbytes, (rows.nbytes, self.nbytes)
        _ck(_load().fhesi_ksk_upload(self.h, _p(rows)))
        return self

    @property
    def nbytes(self) -> int:
        return _load().fhesi_ksk_bytes(self.h)

    @property
    def device_ptr(self) -> int:
        return _load().fhesi_ksk_device_ptr(self.h)

    def download(self) -> np.ndarray:
        out = np.zeros((2, self.ncomp * self.ndigits, self.ctx.L, self.ctx.phim), dtype=np.uint64)
        _ck(_load().fhesi_ksk_download(self.h, _p(out)))
        return out

    def init_batch(self, src, dst_t: "DoubleCRT", logQ: int, a: np.ndarray, err: np.ndarray, decomp_bytes: int = 3):
        """KeySwitchSI::Init (FHE-SI.cpp:153-209) for all columns at once: src = the source key's DoubleCRT components, a = the random
        polynomials [ncol][phim][nlimbs], err = the Gaussian errors [ncol][phim], drawn by the caller in the reference's order."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        err = np.ascontiguousarray(err, dtype=np.int64)
        assert a.shape[0] == err.shape[0] == self.ncomp * self.ndigits
        hs = (_vp * len(src))(*[d.h for d in src])
        _ck(_load().fhesi_keyswitch_init_batch(self.h, hs, len(src), dst_t.h, logQ, decomp_bytes, _p(a), a.shape[-1], _p(err)))
        return self

    def init_batch_seeded(self, src, dst_t: "DoubleCRT", logQ: int, seed: int, public_seed: int, first_index: int, decomp_bytes: int = 3):
        """KeySwitchSI::Init with the column randomness drawn on the device -- philox.h: the public polynomials a from (public_seed, first_index +
        column), the secret errors from (seed, first_index + column).  No default index: an (seed, index) pair must never be used twice."""
        if public_seed == seed:
            raise ValueError("public_seed must differ from the secret seed")
        hs = (_vp * len(src))(*[d.h for d in src])
        _ck(_load().fhesi_keyswitch_init_batch_seeded(self.h, hs, len(src), dst_t.h, logQ, decomp_bytes, seed, public_seed, first_index))
        return self

    FORMS = {-1: "none yet", 0: "per chain prime", 1: "four 30-bit auxiliary primes, limbs", 2: "two largest chain primes, limbs", 3: "two largest chain primes, residues"}

    def form(self):
        """(form, rows, limb_bits) of the last key switch with this matrix (fhesi_ksk_form): which exact form of the dot product ran."""
        f, r, b = C.c_int32(), C.c_int32(), C.c_int32()
        _ck(_load().fhesi_ksk_form(self.h, C.byref(f), C.byref(r), C.byref(b)))
        return f.value, r.value, b.value

    def key_bits(self):
        """(centred, nb) of the last table built from this matrix (fhesi_ksk_key_bits): centred limbs of a generated matrix, and the measured
        size of its integer coefficients."""
        c, b = C.c_int32(), C.c_int32()
        _ck(_load().fhesi_ksk_key_bits(self.h, C.byref(c), C.byref(b)))
        return bool(c.value), b.value

    def hoist(self, k: int) -> "KeySwitchMatrix":
        """The derived matrix sigma_k^-1(self) of the hoisted rotations (fhesi_ksk_hoist): self is the matrix of the automorphism k (source key
        (1, s(X^k))); the result goes to Context.ct_rotations_dev / ct_matvec_dev with the same k and is an ordinary matrix everywhere else."""
        out = KeySwitchMatrix.__new__(KeySwitchMatrix)
        out.ctx, out.ncomp, out.ndigits, out.h, out.k = self.ctx, self.ncomp, self.ndigits, _vp(), int(k)
        _ck(_load().fhesi_ksk_hoist(self.h, int(k), C.byref(out.h)))
        return out

    def mark_dirty(self):
        """The rows were written through device_ptr (e.g. by a collective): derived tables are rebuilt at the next key switch."""
        _ck(_load().fhesi_ksk_mark_dirty(self.h))

    def upload_dev(self, src_ptr: int):
        """Whole matrix from another HBM buffer of the same device (the staging tensor of an RCCL broadcast)."""
        _ck(_load().fhesi_ksk_upload_dev(self.h, _vp(src_ptr)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _load().fhesi_ksk_free(self.h)
                self.h = None
        except Exception:
            pass
