"""ctypes loader for libjampack_amd.so (HIP kernels + C ABI, include/jampack_abi.h).

There is no CPU fallback: if the shared library is missing the import fails loudly, and if no gfx950 device is
visible every call raises JampackError(JPK_E_NODEVICE).
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# JPK_LIB=<path>: another build of the library for THIS process (tools/ab_*.sh alternate two builds on one box without touching the
# product file in place)
LIB_PATH = os.environ.get("JPK_LIB") or os.path.join(HERE, "libjampack_amd.so")

TRAILER = 480
CHUNK = 1 << 20

JPK_OK, JPK_E_ARG, JPK_E_CAPACITY, JPK_E_CORRUPT, JPK_E_DEVICE, JPK_E_ALLOC, JPK_E_NODEVICE = 0, -1, -2, -3, -4, -5, -6


class JampackError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = lib().jpk_strerror(status).decode() if _lib is not None else str(status)
        super().__init__(f"{what}: {msg} ({status})" if what else f"{msg} ({status})")


class Stats(C.Structure):
    _fields_ = [("sa_rounds", C.c_int32), ("sa_key_depth", C.c_int32), ("sa_sorted_elems", C.c_int64),
                ("inv_splitters", C.c_int64), ("inv_overflow_slots", C.c_int64), ("workspace_bytes", C.c_int64),
                ("ans_chunks", C.c_int64), ("ans_rle_symbols", C.c_int64),
                ("sa_round_active", C.c_int32 * 40), ("sa_round_large", C.c_int32 * 40),
                ("enc_chain_cycles", C.c_int64), ("enc_chain_ns", C.c_int64), ("enc_chain_steps", C.c_int64), ("sa_pair_rounds", C.c_int64),
                ("sa_key_order", C.c_int32), ("reserved0", C.c_int32)]


_lib = None

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_vp = C.c_void_p

_SIGS = {
    "jpk_ctx_create": (C.c_int, [C.POINTER(_vp), C.c_int, _vp]),
    "jpk_ctx_destroy": (None, [_vp]),
    "jpk_ctx_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "jpk_ctx_reserve": (C.c_int, [_vp, C.c_int64]),
    "jpk_ctx_profile": (C.c_int, [_vp, C.c_int]),
    "jpk_ctx_profile_count": (C.c_int, []),
    "jpk_ctx_profile_name": (C.c_char_p, [C.c_int]),
    "jpk_ctx_profile_get": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "jpk_device_count": (C.c_int, []),
    "jpk_init": (C.c_int, [C.c_uint64]),
    "jpk_init_devices": (C.c_int, [_i32p, C.c_int32]),
    "jpk_thread_device": (C.c_int, []),
    "jpk_shutdown": (None, []),
    "jpk_release_idle": (C.c_int, []),
    "jpk_strerror": (C.c_char_p, [C.c_int]),
    "jpk_version": (C.c_char_p, []),
    "jpk_bwt_forward": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_bwt_inverse": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p, C.c_int32, C.c_int32]),
    "jpk_ans_encode": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_ans_decode": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p, C.c_int32]),
    "jpk_ans_decoded_size": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64), _i32p]),
    "jpk_rank_encode": (C.c_int, [_vp, _vp, C.c_int32]),
    "jpk_rank_decode": (C.c_int, [_vp, _vp, C.c_int32]),
    "jpk_block_compress": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_block_decompress": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_checksum": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_uint32)]),
    "jpk_jam_block_write": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_jam_block_read": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p, _i32p]),
    "jpk_lz77_decompress": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_lpx_decode": (C.c_int, [_vp, C.c_int32, _vp]),
    "jpk_lpx_encode": (C.c_int, [_vp, C.c_int32, _vp]),
    "jpk_filters_decode": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_checksum_host": (C.c_uint32, [_vp, C.c_int32]),
    "jpk_jam_cli_block_read": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p, _i32p]),
    "jpk_cli_stages_bound": (C.c_int64, [C.c_int64]),
    "jpk_cli_stages_encode": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_jam_cli_block_write": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_lz77_dedupe": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_cli_stages_encode_ex": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p, C.c_uint32]),
    "jpk_filters_encode": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_filters_cost": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "jpk_jam_cli_block_write_ex": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, _i32p, C.c_uint32]),
    "jpk_dev_bwt_forward": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_dev_bwt_inverse": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_dev_bwt_inverse_chains120": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p, C.POINTER(C.c_float)]),
    "jpk_dev_ans_encode": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_dev_ans_decode": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_dev_rank_encode": (C.c_int, [_vp, _vp, _vp, C.c_int32]),
    "jpk_dev_rank_decode": (C.c_int, [_vp, _vp, _vp, C.c_int32]),
    "jpk_dev_block_compress": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_dev_block_decompress": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_dev_blocks_ans_decode": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_dev_blocks_decompress": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_dev_blocks_compress": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p, C.c_int32]),
    "jpk_dev_checksum": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(C.c_uint32)]),
    "jpk_dev_jam_block_write": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, _i32p]),
    "jpk_dev_jam_block_read": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, _i32p, _i32p]),
    "jpk_dev_checksums": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(C.c_uint32)]),
    "jpk_jam_compress_bound": (C.c_int64, [C.c_int64, C.c_int32]),
    "jpk_dev_jam_compress": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32]),
    "jpk_dev_jam_decompress": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_jam_compress": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32]),
    "jpk_jam_decompress": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_jam_frames": (C.c_int, [_vp, C.c_int64, _i32p, C.POINTER(C.c_int64), _i32p]),
    "jpk_dev_jam_index_create": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(_vp), _i32p]),
    "jpk_jam_index_create": (C.c_int, [_vp, C.c_int64, C.POINTER(_vp), _i32p]),
    "jpk_dev_jam_cli_index_create": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(_vp), _i32p]),
    "jpk_jam_cli_index_create": (C.c_int, [_vp, C.c_int64, C.POINTER(_vp), _i32p]),
    "jpk_jam_index_kind": (C.c_int, [_vp]),
    "jpk_dev_jam_cli_decompress_ix": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p, C.POINTER(_vp)]),
    "jpk_jam_index_info": (C.c_int, [_vp, _i32p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "jpk_jam_index_frame": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i32p]),
    "jpk_jam_index_destroy": (None, [_vp]),
    "jpk_dev_jam_read": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_vp), _i32p, _i32p]),
    "jpk_jam_read": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_vp), _i32p, _i32p]),
    "jpk_dev_blocks_lz77_decompress": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_dev_blocks_lpx_decode": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p]),
    "jpk_dev_blocks_filters_decode": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_dev_blocks_lpx_encode": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p]),
    "jpk_dev_blocks_cli_stages_encode": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_jam_cli_compress_bound": (C.c_int64, [C.c_int64, C.c_int32]),
    "jpk_dev_jam_cli_compress": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32]),
    "jpk_jam_cli_compress": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32]),
    "jpk_dev_blocks_lz77_dedupe": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_dev_blocks_cli_stages_encode_ex": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p, C.c_uint32]),
    "jpk_dev_blocks_filters_encode": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_dev_jam_cli_compress_ex": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_uint32]),
    "jpk_jam_cli_compress_ex": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_uint32]),
    "jpk_dev_jam_cli_decompress": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_jam_cli_decompress": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_jam_cli_frames": (C.c_int, [_vp, C.c_int64, _i32p, C.POINTER(C.c_int64), _i32p]),
    "jpk_jam_staged_block_write": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, _i32p, C.c_uint32]),
    "jpk_jam_staged_block_read": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _i32p, _i32p]),
    "jpk_jam_staged_compress_bound": (C.c_int64, [C.c_int64, C.c_int32]),
    "jpk_dev_jam_staged_compress": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_uint32]),
    "jpk_jam_staged_compress": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.c_int32, C.c_uint32]),
    "jpk_jam_staged_frames": (C.c_int, [_vp, C.c_int64, _i32p, C.POINTER(C.c_int64), _i32p]),
    "jpk_dev_jam_staged_decompress": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_jam_staged_decompress": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_dev_blocks_lz77_expand": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_debug_lz77_expand_last": (C.c_int, [_vp, _i32p, _i32p]),
    "jpk_dev_blocks_lz77_expand_deep": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, C.POINTER(_vp), _i32p, _i32p, _i32p]),
    "jpk_debug_lz77_deep_last": (C.c_int, [_vp, _i32p, _i32p]),
    "jpk_debug_lz77_deep_limits": (C.c_int, [_i32p, _i32p, _i32p]),
    "jpk_lz77_size": (C.c_int, [_vp, C.c_int32, C.c_int32, _i32p]),
    "jpk_dev_blocks_lz77_sizes": (C.c_int, [_vp, C.c_int32, C.POINTER(_vp), _i32p, _i32p, _i32p, _i32p]),
    "jpk_dev_jam_staged_index_create": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(_vp), _i32p]),
    "jpk_jam_staged_index_create": (C.c_int, [_vp, C.c_int64, C.c_int32, C.POINTER(_vp), _i32p]),
    "jpk_jam_index_frame_kind": (C.c_int, [_vp, C.c_int32]),
    "jpk_dev_jam_staged_decompress_ix": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p, C.POINTER(_vp)]),
    "jpk_dev_jam_index_recover": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_vp), _i32p]),
    "jpk_jam_index_recover": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_vp), _i32p]),
    "jpk_jam_index_gaps": (C.c_int, [_vp]),
    "jpk_jam_index_gap": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_dev_jam_salvage": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_jam_salvage": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _i32p]),
    "jpk_dev_jam_repair": (C.c_int, [_vp, _vp, _vp, C.c_int64, _i32p, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p]),
    "jpk_jam_repair": (C.c_int, [_vp, _vp, C.c_int64, _i32p, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p]),
    "jpk_jam_update_bound": (C.c_int64, [_vp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.c_int32]),
    "jpk_dev_jam_update": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_vp), _vp, C.c_int64, C.c_int32,
                                     C.c_uint32, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_vp), _i32p, _i32p]),
    "jpk_jam_update": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(_vp), _vp, C.c_int64, C.c_int32,
                                 C.c_uint32, C.c_int32, _vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_vp), _i32p, _i32p]),
    "jpk_debug_jam_scan": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), _i32p]),
    "jpk_debug_jam_recover_limits": (C.c_int, [C.c_int64, C.c_int32]),
    "jpk_dev_suffix_array": (C.c_int, [_vp, _vp, C.c_int32, _vp]),
    "jpk_dev_sort_pairs_u64": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32]),
    "jpk_dev_exclusive_scan_u32": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(C.c_uint32)]),
    "jpk_dev_rle_encode": (C.c_int, [_vp, _vp, C.c_int32, _vp, _i32p]),
    "jpk_dev_model_pairs": (C.c_int, [_vp, _vp, C.c_int32, _vp]),
    "jpk_debug_compress_inflight": (C.c_int, [C.c_int, C.c_int]),
    "jpk_debug_enc_groups": (C.c_int, [C.c_int, C.c_int32]),
    "jpk_debug_arena_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "jpk_debug_combiner_last_batch": (C.c_int, [C.c_int]),
    "jpk_debug_combiner_fail_next": (C.c_int, [C.c_int]),
    "jpk_blocks_compress_multi": (C.c_int, [C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "jpk_blocks_compress_multi_ex": (C.c_int, [C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]),
    "jpk_blocks_decompress_multi": (C.c_int, [C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "jpk_debug_group_fail_next": (C.c_int, [C.c_int]),
    "jpk_debug_multi_plan": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_void_p]),
    "jpk_debug_multi_lock_probe": (C.c_int, [C.c_uint64, C.c_int32]),
    "jpk_debug_group_plan": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "jpk_debug_inv_batch_plan": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "jpk_debug_pair_schedule": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
}

ABI_SYMBOLS = tuple(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
                "or make -C jampack_amd/csrc). jampack_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(l, name)      # AttributeError if the ABI is incomplete
            except AttributeError:
                # an OLDER build chosen through JPK_LIB (the A/B scripts compare a previous round's library on the same box) may lack the
                # newest host-logic probes; the product library must export everything
                if os.environ.get("JPK_LIB") and name.startswith("jpk_debug_"):
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib
