"""ctypes binding of the engine's C ABI (include/resql_hip.h -> resql_amd/libresql_hip.so).

This is the whole Python side of the product: load the library, hand plans and columns across the
C ABI, read results back.  There is no Python or CPU implementation of any operator here — if the
library is missing the import fails, and on a machine without a GPU only compile-only contexts
(device = -1) can be created.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import plan as P

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libresql_hip.so")

STATUS = {0: "OK", 1: "INVALID", 2: "TYPE", 3: "UNSUPPORTED", 4: "DEVICE", 5: "RUNTIME", 6: "NOMEM"}


class rsq_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32),
                ("print_assembly", C.c_int32), ("print_flounder", C.c_int32), ("print_performance", C.c_int32),
                ("num_threads", C.c_int32), ("emit_machine_code", C.c_int32), ("optimize", C.c_int32),
                ("device", C.c_int32), ("kernel_cache_dir", C.c_char_p), ("emission_order", C.c_int32),
                ("compat_flags", C.c_uint32), ("engine_flags", C.c_uint32), ("reserved0", C.c_uint32),
                ("arena_reserve_bytes", C.c_int64), ("arena_keep_bytes", C.c_int64), ("nested_loops_max_pairs", C.c_int64),
                ("nested_loops_inner_slices", C.c_int32), ("tbl_ingest", C.c_int32)]

    @classmethod
    def make(cls, device: int, cache_dir=None, print_source: bool = False, emission_order: int = 0, compat_flags: int = 0,
             engine_flags: int = 0, arena_reserve_bytes: int = 0, arena_keep_bytes: int = 0, nested_loops_max_pairs: int = 0,
             nested_loops_inner_slices: int = 0, tbl_ingest: int = 0):
        return cls(C.sizeof(cls), 1 if print_source else 0, 0, 0, 1, 1, 0, device, cache_dir, emission_order, compat_flags,
                   engine_flags, 0, arena_reserve_bytes, arena_keep_bytes, nested_loops_max_pairs, nested_loops_inner_slices, tbl_ingest)


class rsq_report(C.Structure):
    _fields_ = [("compilation_time_ms", C.c_double), ("execution_time_ms", C.c_double),
                ("kernel_time_ms", C.c_double), ("finalize_time_ms", C.c_double),
                ("num_kernels", C.c_uint64), ("bytes_read", C.c_uint64), ("hbm_gbps", C.c_double),
                ("jit_cache_hits", C.c_int32), ("jit_compiles", C.c_int32)]


class _Report(C.Structure):
    """a report struct of the C ABI as a dict: struct_size and the reserved fields dropped, arrays as lists"""

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size" and not k.startswith("reserved")}
        return {k: list(v) if isinstance(v, C.Array) else v for k, v in d.items()}


def _report_of(ctx, cls, fn: str, handle) -> dict:
    """the report `cls` that the library's `fn` fills for a query or database handle, as a dict"""
    r = cls(C.sizeof(cls))
    ctx._check(getattr(ctx._L, fn)(handle, C.byref(r)))
    return r.as_dict()


class rsq_tbl_load_options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("chunk_bytes", C.c_int64), ("max_device_text_bytes", C.c_int64)]


class rsq_tbl_load_report(_Report):
    _fields_ = [("struct_size", C.c_uint32), ("path", C.c_int32), ("fallback_reason", C.c_int32), ("reserved", C.c_int32),
                ("rows", C.c_int64), ("text_bytes", C.c_int64), ("lines_patched", C.c_int64),
                ("read_ms", C.c_double), ("copy_ms", C.c_double), ("kernel_ms", C.c_double), ("patch_ms", C.c_double),
                ("stats_ms", C.c_double), ("total_ms", C.c_double),
                ("count_kernel_ms", C.c_double), ("starts_kernel_ms", C.c_double), ("parse_kernel_ms", C.c_double)]


TBL_HOST, TBL_DEVICE = 1, 2      # rsq_tbl_load_options.mode (0: the context's tbl_ingest)
# rsq_tbl_fallback: why a load that asked for the device took the host path
TBL_FALLBACK_NONE, TBL_FALLBACK_NO_DEVICE, TBL_FALLBACK_COLUMNS, TBL_FALLBACK_TERMINATOR, TBL_FALLBACK_DOES_NOT_FIT, TBL_FALLBACK_ODD_LINES = range(6)


class rsq_rowstore_options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("chunk_bytes", C.c_int64)]


class rsq_rowstore_report(_Report):
    _fields_ = [("struct_size", C.c_uint32), ("path", C.c_int32), ("fallback_reason", C.c_int32), ("reserved", C.c_int32),
                ("rows", C.c_int64), ("tuple_bytes", C.c_int64), ("chunks", C.c_int64),
                ("stage_ms", C.c_double), ("copy_ms", C.c_double), ("kernel_ms", C.c_double), ("transpose_ms", C.c_double),
                ("stats_ms", C.c_double), ("total_ms", C.c_double)]


ROWSTORE_HOST, ROWSTORE_DEVICE = 1, 2      # rsq_rowstore_options.mode (0: the context's set_rowstore_bridge)
# rsq_rowstore_fallback: why a bridge that asked for the device transposed on the host
ROWSTORE_FALLBACK_NONE, ROWSTORE_FALLBACK_NO_DEVICE, ROWSTORE_FALLBACK_COLUMNS = range(3)


class rsq_result_text_options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("chunk_rows", C.c_int64), ("max_device_bytes", C.c_int64)]


class rsq_result_text_report(_Report):
    _fields_ = [("struct_size", C.c_uint32), ("path", C.c_int32), ("fallback_reason", C.c_int32), ("tuples_from_device", C.c_int32),
                ("rows", C.c_int64), ("text_bytes", C.c_int64), ("chunks", C.c_int64),
                ("upload_ms", C.c_double), ("kernel_ms", C.c_double), ("download_ms", C.c_double), ("total_ms", C.c_double)]


TEXT_HOST, TEXT_DEVICE = 1, 2      # rsq_result_text_options.mode (0: the context's set_result_text)
# rsq_text_fallback: why a result text that asked for the device was written by the host
TEXT_FALLBACK_NONE, TEXT_FALLBACK_NO_DEVICE, TEXT_FALLBACK_SCHEMA, TEXT_FALLBACK_DOES_NOT_FIT = range(4)


class rsq_order_limit_report(_Report):
    _fields_ = [("struct_size", C.c_uint32), ("planned", C.c_int32), ("path", C.c_int32), ("fallback_reason", C.c_int32),
                ("first_key_column", C.c_int32), ("key_is32", C.c_int32), ("descending", C.c_int32), ("reserved", C.c_int32),
                ("rows", C.c_int64), ("want", C.c_int64), ("candidates", C.c_int64), ("capacity", C.c_int64),
                ("select_ms", C.c_double), ("copy_ms", C.c_double), ("tail_ms", C.c_double)]


ORDER_LIMIT_HOST, ORDER_LIMIT_DEVICE = 0, 1      # Context.set_order_limit
# rsq_order_limit_fallback: why an execution under set_order_limit(1) sorted every row on the host
(ORDER_LIMIT_FALLBACK_NONE, ORDER_LIMIT_FALLBACK_SHAPE, ORDER_LIMIT_FALLBACK_FEW_ROWS, ORDER_LIMIT_FALLBACK_OVERFLOW,
 ORDER_LIMIT_FALLBACK_TIES) = range(5)


class rsq_result_pack_report(_Report):
    _fields_ = [("struct_size", C.c_uint32), ("planned", C.c_int32), ("path", C.c_int32), ("fallback_reason", C.c_int32),
                ("sorted_on_host", C.c_int32), ("tuple_size", C.c_int32), ("rows", C.c_int64), ("tuple_bytes", C.c_int64),
                ("kernel_ms", C.c_double), ("copy_ms", C.c_double), ("sort_ms", C.c_double)]


RESULT_PACK_HOST, RESULT_PACK_DEVICE = 0, 1      # Context.set_result_pack
# rsq_result_pack_fallback: why an execution under set_result_pack(1) packed its result tuples on the host
(RESULT_PACK_FALLBACK_NONE, RESULT_PACK_FALLBACK_SHAPE, RESULT_PACK_FALLBACK_SMALL, RESULT_PACK_FALLBACK_DOES_NOT_FIT,
 RESULT_PACK_FALLBACK_ORDER_LIMIT) = range(5)


class rsq_order_sort_report(_Report):
    _fields_ = [("struct_size", C.c_uint32), ("planned", C.c_int32), ("path", C.c_int32), ("fallback_reason", C.c_int32),
                ("keys", C.c_int32), ("key_bits", C.c_int32 * 8), ("total_bits", C.c_int32), ("words", C.c_int32), ("passes", C.c_int32),
                ("tuple_size", C.c_int32), ("reserved", C.c_int32), ("rows", C.c_int64), ("lead", C.c_int64), ("out_rows", C.c_int64),
                ("tied_pairs", C.c_int64), ("range_ms", C.c_double), ("sort_ms", C.c_double), ("pack_ms", C.c_double),
                ("gather_ms", C.c_double), ("copy_ms", C.c_double)]


ORDER_SORT_HOST, ORDER_SORT_DEVICE = 0, 1      # Context.set_order_sort
# rsq_order_sort_fallback: why an execution under set_order_sort(1) sorted its tuples on the host
(ORDER_SORT_FALLBACK_NONE, ORDER_SORT_FALLBACK_SHAPE, ORDER_SORT_FALLBACK_SMALL, ORDER_SORT_FALLBACK_DOES_NOT_FIT,
 ORDER_SORT_FALLBACK_TIES, ORDER_SORT_FALLBACK_ORDER_LIMIT) = range(6)


class rsq_memory_stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32), ("device_slab_bytes", C.c_uint64), ("device_used_bytes", C.c_uint64),
                ("device_slab_allocs", C.c_uint64), ("pinned_slab_bytes", C.c_uint64), ("pinned_used_bytes", C.c_uint64),
                ("pinned_slab_allocs", C.c_uint64), ("raw_driver_calls", C.c_uint64), ("arena_requests", C.c_uint64), ("driver_ms", C.c_double),
                ("plan_memo_entries", C.c_uint64), ("plan_memo_hits", C.c_uint64), ("key_index_entries", C.c_uint64), ("key_index_bytes", C.c_uint64),
                ("column_image_bytes", C.c_uint64)]


class rsq_multi_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_devices", C.c_int32), ("base", C.POINTER(rsq_config)), ("devices", C.POINTER(C.c_int32)),
                ("merge", C.c_int32), ("reserved0", C.c_int32)]


MERGE_AUTO, MERGE_RCCL, MERGE_PEER_COPY = 0, 1, 2
EMIT_REFERENCE, EMIT_ANY = 0, 1
COMPAT_JIT_INT16_CAST = 1      # rsq_compat: TYPECAST INT -> BIGINT as the reference's asmjit JIT executes it (low 16 bits)
ENGINE_DRIVER_ALLOC, ENGINE_NO_PLAN_MEMO, ENGINE_NESTED_LOOPS, ENGINE_DERIVED_MULTI, ENGINE_DICT_MULTI = 1, 2, 4, 8, 16      # rsq_engine_flags


class EngineError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"[{STATUS.get(status, status)}] {message}")
        self.status = status
        self.message = message


_lib = None


def lib():
    """load libresql_hip.so; raises if it has not been built (no fallback)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C resql_amd/csrc` "
                              f"(or __graft_entry__.build()); the engine has no Python/CPU fallback")
        # PyTorch-ROCm wheels bundle their own HIP runtime.  If this library brings the system runtime up first and
        # torch is imported later in the same process (multi-GPU merge, torch.distributed), torch's copy reports
        # "No HIP GPUs are available".  Loading torch's runtime first makes both share it.  Skipped when torch is not
        # installed or RSQ_NO_TORCH_PRELOAD is set (pure C/C++ hosts never see this).
        if "torch" not in __import__("sys").modules and not os.environ.get("RSQ_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.rsq_ctx_create.argtypes = [C.POINTER(rsq_config), C.POINTER(vp)]
        L.rsq_ctx_destroy.argtypes = [vp]
        L.rsq_last_error.restype = C.c_char_p
        L.rsq_ctx_memory_stats.argtypes = [vp, C.POINTER(rsq_memory_stats)]
        L.rsq_last_error.argtypes = [vp]
        L.rsq_table_create.argtypes = [vp, C.POINTER(P.rsq_table_desc), C.POINTER(vp)]
        L.rsq_table_create_device.argtypes = [vp, C.POINTER(P.rsq_table_desc), C.POINTER(vp)]
        L.rsq_table_from_rowstore.argtypes = [vp, C.POINTER(P.rsq_table_desc), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t), i32, C.POINTER(vp)]
        L.rsq_table_from_rowstore_ex.argtypes = [vp, C.POINTER(P.rsq_table_desc), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), i32,
                                                 C.POINTER(rsq_rowstore_options), C.POINTER(rsq_rowstore_report), C.POINTER(vp)]
        L.rsq_ctx_set_rowstore_bridge.argtypes = [vp, i32]
        L.rsq_table_generate.argtypes = [vp, i32, i64, i64, C.c_double, i64, C.c_uint64, C.POINTER(vp)]
        L.rsq_table_load_tbl.argtypes = [vp, C.POINTER(P.rsq_table_desc), C.c_char_p, C.c_char, i32, C.POINTER(vp)]
        L.rsq_table_load_tbl_ex.argtypes = [vp, C.POINTER(P.rsq_table_desc), C.c_char_p, C.c_char, i32, C.POINTER(rsq_tbl_load_options),
                                            C.POINTER(rsq_tbl_load_report), C.POINTER(vp)]
        L.rsq_table_rows.restype = i64
        L.rsq_table_rows.argtypes = [vp]
        L.rsq_table_read_column.argtypes = [vp, vp, C.c_char_p, vp, C.c_size_t]
        L.rsq_table_read_image.argtypes = [vp, vp, C.c_char_p, i32, vp, C.c_size_t, C.POINTER(i64)]
        L.rsq_table_set_first_row.argtypes = [vp, i64]
        L.rsq_table_refresh_stats.argtypes = [vp]
        L.rsq_table_append.argtypes = [vp, vp]
        L.rsq_table_stats_bytes.restype = i64
        L.rsq_table_stats_bytes.argtypes = [vp]
        L.rsq_table_stats_export.argtypes = [vp, vp, i64]
        L.rsq_table_unify_shard_stats.argtypes = [vp, vp, i32, i64]
        L.rsq_table_unify_shard_dictionaries.argtypes = [C.POINTER(vp), i32]
        L.rsq_table_time_dictionary_pass.argtypes = [vp, C.c_char_p, i32, C.POINTER(C.c_double)]
        L.rsq_table_total_rows.restype = i64
        L.rsq_table_total_rows.argtypes = [vp]
        L.rsq_table_destroy.argtypes = [vp]
        L.rsq_query_compile.argtypes = [vp, C.POINTER(P.rsq_plan_desc), C.POINTER(vp), i32, C.POINTER(vp)]
        L.rsq_query_execute.argtypes = [vp]
        L.rsq_query_await_kernels.argtypes = [vp]
        L.rsq_query_execute_partial.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.rsq_query_execute_partial_async.argtypes = [vp]
        L.rsq_ctx_set_stream.argtypes = [vp, vp, i32]
        L.rsq_query_finalize.argtypes = [vp]
        L.rsq_query_bind_partial.argtypes = [vp, vp, C.c_size_t]
        L.rsq_query_merge_gathered.argtypes = [vp, vp, i32]
        L.rsq_query_finalize_host.argtypes = [vp, C.POINTER(i64), i64]
        L.rsq_query_partial_layout.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.rsq_query_result.argtypes = [vp, C.POINTER(P.rsq_result_view)]
        L.rsq_query_report.argtypes = [vp, C.POINTER(rsq_report)]
        L.rsq_query_kernel_time_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int32]
        L.rsq_query_nested_loops_slices.argtypes = [vp, C.POINTER(i32)]
        L.rsq_nested_loops_slices.restype = i32
        L.rsq_nested_loops_slices.argtypes = [i64, i64, i64, i32]
        L.rsq_query_source.restype = C.c_char_p
        L.rsq_query_source.argtypes = [vp]
        L.rsq_query_explain.restype = C.c_char_p
        L.rsq_query_explain.argtypes = [vp]
        L.rsq_query_destroy.argtypes = [vp]
        L.rsq_serialize_expr.restype = vp
        L.rsq_serialize_expr.argtypes = [vp, C.POINTER(P.rsq_plan_desc), i32, i32, C.POINTER(vp), i32]
        L.rsq_result_serialize.restype = vp
        L.rsq_result_serialize.argtypes = [C.POINTER(P.rsq_result_view)]
        L.rsq_free.argtypes = [vp]
        L.rsq_query_result_text.argtypes = [vp, C.POINTER(rsq_result_text_options), C.POINTER(rsq_result_text_report), C.POINTER(vp), C.POINTER(i64)]
        L.rsq_query_result_write.argtypes = [vp, C.c_char_p, C.POINTER(rsq_result_text_options), C.POINTER(rsq_result_text_report)]
        L.rsq_ctx_set_result_text.argtypes = [vp, i32]
        L.rsq_ctx_set_row_cells.argtypes = [vp, i32]
        L.rsq_db_result_text_report.argtypes = [vp, C.POINTER(rsq_result_text_report)]
        L.rsq_ctx_set_order_limit.argtypes = [vp, i32]
        L.rsq_query_order_limit_report.argtypes = [vp, C.POINTER(rsq_order_limit_report)]
        L.rsq_db_order_limit_report.argtypes = [vp, C.POINTER(rsq_order_limit_report)]
        L.rsq_prim_column_topk.argtypes = [vp, vp, i32, i64, i32, i64, i64, vp, i32, vp, vp, vp, vp, vp]
        L.rsq_ctx_set_result_pack.argtypes = [vp, i32]
        L.rsq_query_result_pack_report.argtypes = [vp, C.POINTER(rsq_result_pack_report)]
        L.rsq_db_result_pack_report.argtypes = [vp, C.POINTER(rsq_result_pack_report)]
        L.rsq_prim_pack_tuples.argtypes = [vp, vp, vp, i32, i64, vp, i64]
        L.rsq_ctx_set_order_sort.argtypes = [vp, i32]
        L.rsq_query_order_sort_report.argtypes = [vp, C.POINTER(rsq_order_sort_report)]
        L.rsq_db_order_sort_report.argtypes = [vp, C.POINTER(rsq_order_sort_report)]
        L.rsq_prim_sort_rows.argtypes = [vp, vp, vp, i32, vp, vp, i32, i64, i64, vp, vp, vp, vp]
        L.rsq_prim_gather_tuples.argtypes = [vp, vp, i32, i64, vp, i64, vp, i64]
        L.rsq_ref_emission_order.argtypes = [vp, i64, C.c_uint64, i32, vp]
        L.rsq_ref_emission_order_device.argtypes = [vp, vp, i64, C.c_uint64, vp]
        L.rsq_prim_exclusive_scan.argtypes = [vp, vp, i64, i32, vp, vp]
        L.rsq_prim_rank_index.argtypes = [vp, vp, i64, i32, vp, vp]
        L.rsq_prim_rank_place.argtypes = [vp, vp, i64, i64, i64, vp, vp, i32, i32, i32, i64, vp, vp]
        L.rsq_prim_radix_sort_pairs.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp]
        L.rsq_prim_running_min.argtypes = [vp, vp, i64, vp, vp]
        L.rsq_prim_merge_group_rows.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
        L.rsq_prim_topk_select.argtypes = [vp, vp, i64, i64, i32, i32, i32, i32, i64, i32, vp, i64, vp, vp, vp]
        L.rsq_measure_read_bandwidth.argtypes = [vp, C.c_size_t, i32, C.POINTER(C.c_double)]
        L.rsq_sql_plan_select.argtypes = [vp, C.c_char_p, C.POINTER(vp), i32, C.POINTER(vp)]
        L.rsq_sql_plan_desc.restype = C.POINTER(P.rsq_plan_desc)
        L.rsq_sql_plan_desc.argtypes = [vp]
        L.rsq_sql_plan_destroy.argtypes = [vp]
        L.rsq_sql_plan_text.restype = vp
        L.rsq_sql_plan_text.argtypes = [vp]
        L.rsq_sql_compile.argtypes = [vp, C.c_char_p, C.POINTER(vp), i32, C.POINTER(vp)]
        L.rsq_sql_describe.restype = vp
        L.rsq_sql_describe.argtypes = [vp, C.c_char_p, i32]
        L.rsq_db_create.argtypes = [vp, C.POINTER(vp)]
        L.rsq_db_execute.argtypes = [vp, C.c_char_p, C.POINTER(i32), C.POINTER(P.rsq_result_view)]
        L.rsq_db_adopt_table.argtypes = [vp, vp]
        L.rsq_db_message.restype = C.c_char_p
        L.rsq_db_message.argtypes = [vp]
        L.rsq_db_report.argtypes = [vp, C.POINTER(rsq_report)]
        L.rsq_db_load_report.argtypes = [vp, C.POINTER(rsq_tbl_load_report)]
        L.rsq_db_destroy.argtypes = [vp]
        L.rsq_multi_create.argtypes = [C.POINTER(rsq_multi_config), C.POINTER(vp)]
        L.rsq_multi_destroy.argtypes = [vp]
        L.rsq_multi_last_error.restype = C.c_char_p
        L.rsq_multi_last_error.argtypes = [vp]
        L.rsq_multi_devices.restype = i32
        L.rsq_multi_devices.argtypes = [vp]
        L.rsq_multi_ctx.restype = vp
        L.rsq_multi_ctx.argtypes = [vp, i32]
        L.rsq_multi_merge_name.restype = C.c_char_p
        L.rsq_multi_merge_name.argtypes = [vp]
        L.rsq_multi_shard_rows.restype = None
        L.rsq_multi_shard_rows.argtypes = [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)]
        L.rsq_multi_table_generate.argtypes = [vp, i32, i64, C.c_double, i64, C.c_uint64, C.POINTER(vp)]
        L.rsq_multi_table_generate_on_key.argtypes = [vp, i32, i64, C.c_double, i64, C.c_uint64, C.c_char_p, C.POINTER(vp)]
        L.rsq_multi_query_merge_name.restype = C.c_char_p
        L.rsq_multi_query_merge_name.argtypes = [vp]
        L.rsq_multi_query_explain.restype = C.c_char_p
        L.rsq_multi_query_explain.argtypes = [vp, i32]
        L.rsq_multi_query_compile.argtypes = [vp, C.POINTER(P.rsq_plan_desc), C.POINTER(vp), i32, C.POINTER(vp)]
        L.rsq_multi_query_execute.argtypes = [vp]
        L.rsq_multi_query_result.argtypes = [vp, C.POINTER(P.rsq_result_view)]
        L.rsq_multi_query_report.argtypes = [vp, C.POINTER(rsq_report), C.POINTER(C.c_double)]
        L.rsq_multi_query_collective_ms.restype = C.c_double
        L.rsq_multi_query_collective_ms.argtypes = [vp]
        L.rsq_multi_query_destroy.argtypes = [vp]
        _lib = L
    return _lib


EXPORTED_SYMBOLS = [
    "rsq_ctx_create", "rsq_ctx_destroy", "rsq_last_error", "rsq_table_create", "rsq_table_create_device",
    "rsq_table_from_rowstore", "rsq_table_from_rowstore_ex", "rsq_ctx_set_rowstore_bridge", "rsq_table_load_tbl", "rsq_table_load_tbl_ex", "rsq_table_generate", "rsq_table_rows", "rsq_table_set_first_row", "rsq_table_refresh_stats", "rsq_table_append", "rsq_ctx_memory_stats", "rsq_table_read_column", "rsq_table_read_image",
    "rsq_table_stats_bytes", "rsq_table_stats_export", "rsq_table_unify_shard_stats", "rsq_table_unify_shard_dictionaries", "rsq_table_time_dictionary_pass", "rsq_table_total_rows",
    "rsq_table_destroy", "rsq_query_compile", "rsq_query_execute", "rsq_query_await_kernels", "rsq_query_execute_partial",
    "rsq_query_execute_partial_async", "rsq_ctx_set_stream",
    "rsq_query_finalize", "rsq_query_merge_gathered", "rsq_query_finalize_host", "rsq_query_bind_partial", "rsq_query_partial_layout", "rsq_query_result", "rsq_query_report", "rsq_query_kernel_time_stats", "rsq_query_nested_loops_slices", "rsq_nested_loops_slices", "rsq_query_source", "rsq_query_explain",
    "rsq_query_destroy", "rsq_serialize_expr", "rsq_result_serialize", "rsq_free", "rsq_query_result_text", "rsq_query_result_write", "rsq_ctx_set_result_text", "rsq_ctx_set_row_cells", "rsq_db_result_text_report", "rsq_ref_emission_order", "rsq_ref_emission_order_device",
    "rsq_prim_exclusive_scan", "rsq_prim_rank_index", "rsq_prim_rank_place",
    "rsq_prim_radix_sort_pairs", "rsq_prim_running_min", "rsq_prim_merge_group_rows", "rsq_prim_topk_select", "rsq_prim_column_topk",
    "rsq_ctx_set_order_limit", "rsq_query_order_limit_report", "rsq_db_order_limit_report",
    "rsq_ctx_set_result_pack", "rsq_query_result_pack_report", "rsq_db_result_pack_report", "rsq_prim_pack_tuples",
    "rsq_ctx_set_order_sort", "rsq_query_order_sort_report", "rsq_db_order_sort_report", "rsq_prim_sort_rows", "rsq_prim_gather_tuples",
    "rsq_measure_read_bandwidth",
    "rsq_sql_plan_select", "rsq_sql_plan_desc", "rsq_sql_plan_destroy", "rsq_sql_plan_text", "rsq_sql_compile", "rsq_sql_describe",
    "rsq_db_create", "rsq_db_execute", "rsq_db_message", "rsq_db_adopt_table", "rsq_db_report", "rsq_db_load_report", "rsq_db_destroy",
    "rsq_multi_create", "rsq_multi_destroy", "rsq_multi_last_error", "rsq_multi_devices", "rsq_multi_ctx", "rsq_multi_merge_name",
    "rsq_multi_shard_rows", "rsq_multi_table_generate", "rsq_multi_table_generate_on_key", "rsq_multi_query_merge_name", "rsq_multi_query_explain", "rsq_multi_query_compile", "rsq_multi_query_execute",
    "rsq_multi_query_result", "rsq_multi_query_report", "rsq_multi_query_collective_ms", "rsq_multi_query_destroy",
]

NLJ_MIN_SLICE_ROWS = 512      # include/resql_hip.h RSQ_NLJ_MIN_SLICE_ROWS: the policy's floor on inner rows per slice


def nested_loops_slices(base_workgroups: int, max_workgroups: int, inner_rows: int, configured: int = 0) -> int:
    """rsq_nested_loops_slices: the slices a launch with these workgroup counts cuts the inner rows of a nested-loops join into"""
    return lib().rsq_nested_loops_slices(base_workgroups, max_workgroups, inner_rows, configured)


def unify_shard_dictionaries(tables: Sequence["DeviceTable"]) -> None:
    """one dictionary per dictionary-coded column for the shards of ONE table held in this process (rsq_table_unify_shard_dictionaries):
    the union of the shards' entries where it has at most 256 values, codes rewritten in place; other columns stay as they are"""
    if not tables:
        raise ValueError("unify_shard_dictionaries: no tables")
    arr = (C.c_void_p * len(tables))(*[t.h for t in tables])
    tables[0].ctx._check(lib().rsq_table_unify_shard_dictionaries(arr, len(tables)))


GEN_LINEITEM, GEN_ORDERS, GEN_CUSTOMER, GEN_SYNTHETIC = 0, 1, 2, 3
RANK_CHUNK_BLOCKS = 1024      # csrc/engine.h RSQ_RANK_CHUNK_BLOCKS: 32-byte bitmap blocks per entry of the rank index's chunk_base


class Context:
    """one engine context per GPU (device=-1: compile-only, no GPU needed)"""

    @classmethod
    def borrowed(cls, handle, device: int) -> "Context":
        """a context owned by someone else (a MultiContext's shard): close() does not destroy it"""
        self = cls.__new__(cls)
        self._L = lib()
        self._cache = None
        self.h = C.c_void_p(handle)
        self.device = device
        self._borrowed = True
        return self

    def __init__(self, device: int = 0, cache_dir: Optional[str] = None, print_source: bool = False, emission_order: int = 0,
                 compat_flags: int = 0, engine_flags: int = 0, arena_reserve_bytes: int = 0, arena_keep_bytes: int = 0,
                 nested_loops_max_pairs: int = 0, nested_loops_inner_slices: int = 0, tbl_ingest: int = 0):
        """emission_order: EMIT_REFERENCE (0: rows of an unsorted aggregation in the reference's hash-table order) or EMIT_ANY;
        compat_flags: rsq_compat bits (COMPAT_JIT_INT16_CAST); engine_flags: rsq_engine_flags bits (ENGINE_DRIVER_ALLOC,
        ENGINE_NO_PLAN_MEMO, ENGINE_NESTED_LOOPS); arena_*, nested_loops_max_pairs (0: 2^36 pairs), nested_loops_inner_slices (0: chosen per execution,
        1: never split, 2..4096: that many slices of an aggregating nested-loops join's inner rows), tbl_ingest (0: BULK INSERT parses its
        text on the host, 1: on the device): see rsq_config"""
        self._L = lib()
        self._cache = cache_dir.encode() if cache_dir else None
        cfg = rsq_config.make(device, self._cache, print_source, emission_order, compat_flags, engine_flags, arena_reserve_bytes, arena_keep_bytes,
                              nested_loops_max_pairs, nested_loops_inner_slices, tbl_ingest)
        h = C.c_void_p()
        rc = self._L.rsq_ctx_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise EngineError(rc, self._L.rsq_last_error(None).decode())
        self.h = h
        self.device = device

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(rc, self._L.rsq_last_error(self.h).decode())

    def memory_stats(self) -> dict:
        """rsq_ctx_memory_stats as a dict: what the context's arenas hold, driver calls, plan-memo entries / hits"""
        m = rsq_memory_stats()
        m.struct_size = C.sizeof(rsq_memory_stats)
        self._check(self._L.rsq_ctx_memory_stats(self.h, C.byref(m)))
        return {k: getattr(m, k) for k, _ in rsq_memory_stats._fields_ if k not in ("struct_size", "reserved0")}

    # ---- device primitives exposed for tests (resql_hip.h rsq_prim_*): numpy arrays in, (results..., notes) out ----
    def prim_scan(self, counts: np.ndarray, form: int):
        """exclusive scan of uint32 counts into uint64 offsets; form 0: three launches, 1: one launch"""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        offsets = np.empty(len(counts), dtype=np.uint64)
        notes = C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_exclusive_scan(self.h, counts.ctypes.data, len(counts), form, offsets.ctypes.data, C.addressof(notes)))
        return offsets, notes.value

    def prim_rank_index(self, blocks: np.ndarray, form: int):
        """rank index of a key bitmap [n_blocks, 8] of uint32 (word 0: rank, 1..7: bits); form 0: two launches, 1: one launch"""
        out = np.array(blocks, dtype=np.uint32, order="C").reshape(-1, 8)
        chunk_base = np.full((len(out) + RANK_CHUNK_BLOCKS - 1) // RANK_CHUNK_BLOCKS + 1, 0xffffffff, dtype=np.uint32)
        notes = C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_rank_index(self.h, out.ctypes.data, len(out), form, chunk_base.ctypes.data, C.addressof(notes)))
        return out, chunk_base, notes.value

    def prim_rank_place(self, blocks: np.ndarray, bm_min: int, bm_bits: int, records: np.ndarray, used: np.ndarray, region: int, n_words: int,
                        capacity: int):
        """records [n_waves * region * n_words] of int64 (word 0 of a record: its key) placed at the rank of their keys: [capacity, n_words]"""
        blocks = np.ascontiguousarray(blocks, dtype=np.uint32).reshape(-1, 8)
        records = np.ascontiguousarray(records, dtype=np.int64)
        used = np.ascontiguousarray(used, dtype=np.uint32)
        if records.size != len(used) * region * n_words:
            raise ValueError("records must hold n_waves * region * n_words words")
        out = np.zeros((capacity, n_words), dtype=np.int64)
        notes = C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_rank_place(self.h, blocks.ctypes.data, len(blocks), bm_min, bm_bits, records.ctypes.data, used.ctypes.data,
                                                len(used), region, n_words, capacity, out.ctypes.data, C.addressof(notes)))
        return out, notes.value

    def prim_radix_sort_pairs(self, keys: np.ndarray, vals: np.ndarray, key_bits: int):
        """(uint64 key, uint32 value) pairs sorted, stably, by the low 8 * ceil(key_bits / 8) bits of the keys: (keys, vals, notes)"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        if len(keys) != len(vals):
            raise ValueError("as many values as keys")
        keys_out, vals_out = np.zeros(len(keys), dtype=np.uint64), np.zeros(len(keys), dtype=np.uint32)
        notes = C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_radix_sort_pairs(self.h, keys.ctypes.data, vals.ctypes.data, len(keys), key_bits, keys_out.ctypes.data,
                                                      vals_out.ctypes.data, C.addressof(notes)))
        return keys_out, vals_out, notes.value

    def prim_running_min(self, values: np.ndarray):
        """out[i] = min(values[0..i]) of int64 values: (out, notes)"""
        values = np.ascontiguousarray(values, dtype=np.int64)
        out = np.zeros(len(values), dtype=np.int64)
        notes = C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_running_min(self.h, values.ctypes.data, len(values), out.ctypes.data, C.addressof(notes)))
        return out, notes.value

    def prim_merge_group_rows(self, rows: np.ndarray, n_tab: int, keys, accs):
        """group rows [n, stride] of int64 ([first row | n_tab table words | accumulators]) merged by key; keys: (word, type tag, len)
        each, accs: (word, kind 0 sum / 2 min / 3 max) each: (the groups' rows [count, stride], notes)"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        n, stride = rows.shape
        kw, kt, kl = (np.array([k[j] for k in keys], dtype=np.int32) for j in range(3))
        aw, ak = (np.array([a[j] for a in accs], dtype=np.int32) for j in range(2))
        out = np.zeros((n, stride), dtype=np.int64)
        count, notes = C.c_uint64(0xffffffffffffffff), C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_merge_group_rows(self.h, rows.ctypes.data, n, stride, n_tab, kw.ctypes.data, kt.ctypes.data, kl.ctypes.data, len(keys),
                                                      aw.ctypes.data, ak.ctypes.data, len(accs), out.ctypes.data, C.addressof(count), C.addressof(notes)))
        if count.value > n:
            raise EngineError(5, f"the merge reports {count.value} groups of {n} rows")
        return out[:count.value], notes.value

    def prim_topk_select(self, rows: np.ndarray, key_word: int, is32: bool, desc: bool, want: int, form: int, capacity: int,
                         rows_upper_bound: Optional[int] = None, image_range=None):
        """ORDER BY ... LIMIT pre-selection over rows [n, stride] of int64; form 0: the exact radix select, 1: the one-histogram form over
        image_range = (largest image, ~smallest image): (cand [capacity, stride], 0xff bytes where nothing was written; count; notes)"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        n, stride = rows.shape
        rng = None if image_range is None else np.array([int(x) & 0xffffffffffffffff for x in image_range], dtype=np.uint64)
        cand = np.zeros((capacity, stride), dtype=np.int64)
        count, notes = C.c_uint32(0xffffffff), C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_topk_select(self.h, rows.ctypes.data, n, n if rows_upper_bound is None else rows_upper_bound, stride, key_word,
                                                 1 if is32 else 0, 1 if desc else 0, want, form, None if rng is None else rng.ctypes.data, capacity,
                                                 cand.ctypes.data, C.addressof(count), C.addressof(notes)))
        return cand, count.value, notes.value

    def prim_column_topk(self, key: np.ndarray, desc: bool, want: int, capacity: int, payload: np.ndarray):
        """ORDER BY ... LIMIT pre-selection over a column (rsq_prim_column_topk): key int32 or int64 [n], payload uint8 [n, width]:
        (positions uint32 [capacity] and payload rows uint8 [capacity, width], 0xff bytes where nothing was written; the number of rows
        with image >= T; T; notes)"""
        key = np.ascontiguousarray(key)
        if key.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
            raise ValueError("prim_column_topk: the key column is int32 or int64")
        payload = np.ascontiguousarray(payload, dtype=np.uint8).reshape(len(key), -1)
        width = payload.shape[1]
        positions = np.zeros(capacity, dtype=np.uint32)
        out = np.zeros((capacity, width), dtype=np.uint8)
        count, threshold, notes = C.c_uint64(0xffffffffffffffff), C.c_uint64(0), C.c_uint32(0xffffffff)
        self._check(self._L.rsq_prim_column_topk(self.h, key.ctypes.data, key.dtype.itemsize, len(key), 1 if desc else 0, want, capacity,
                                                 payload.ctypes.data, width, positions.ctypes.data, out.ctypes.data, C.addressof(count),
                                                 C.addressof(threshold), C.addressof(notes)))
        return positions, out, count.value, threshold.value, notes.value

    def prim_pack_tuples(self, columns, types) -> np.ndarray:
        """the materialisation's device tail over host columns (rsq_prim_pack_tuples): columns[c] the cells of types[c] (plan.SqlType) as
        a contiguous array of n_rows x width bytes; returns the device's buffer as uint8 [n_rows * tuple size + 64] - the packed tuples
        and, behind them, 64 guard bytes that are still 0xEE where the kernel kept to its range"""
        cols = [np.ascontiguousarray(c).view(np.uint8).reshape(-1) for c in columns]
        if len(cols) != len(types) or not cols:
            raise ValueError("prim_pack_tuples: one column per type")
        n = len(cols[0]) // types[0].width
        for c, t in zip(cols, types):
            if len(c) != n * t.width:
                raise ValueError("prim_pack_tuples: every column holds n_rows cells of its type's width")
        ts = sum(2 if (t.tag == P.CHAR and t.len == 1) else t.width + 1 if t.tag in (P.CHAR, P.VARCHAR) else t.width for t in types)
        out = np.zeros(n * ts + 64, dtype=np.uint8)
        ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        ctypes_ = (P.rsq_type * len(types))(*[t.c() for t in types])
        self._check(self._L.rsq_prim_pack_tuples(self.h, ptrs, ctypes_, len(types), n, out.ctypes.data, len(out)))
        return out

    def prim_sort_rows(self, columns, types, key_columns, descending, lead=None):
        """the device's order of column-wise rows (rsq_prim_sort_rows): columns[c] the cells of types[c] (plan.SqlType) as a contiguous
        array of n_rows x width bytes, key_columns / descending the sort keys.  Returns (perm uint32 [n_rows], tied pairs among the
        leading `lead` rows (default: all), bits per key [8], 64-bit words of the composite key)"""
        cols = [np.ascontiguousarray(c).view(np.uint8).reshape(-1) for c in columns]
        if len(cols) != len(types) or not cols or len(key_columns) != len(descending):
            raise ValueError("prim_sort_rows: one column per type, one direction per key")
        n = len(cols[0]) // types[0].width
        for c, t in zip(cols, types):
            if len(c) != n * t.width:
                raise ValueError("prim_sort_rows: every column holds n_rows cells of its type's width")
        perm = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
        ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        ctypes_ = (P.rsq_type * len(types))(*[t.c() for t in types])
        kc = (C.c_int32 * len(key_columns))(*key_columns)
        kd = (C.c_int32 * len(descending))(*[1 if d else 0 for d in descending])
        ties, words, bits = C.c_int64(-1), C.c_int32(-1), (C.c_int32 * 8)()
        self._check(self._L.rsq_prim_sort_rows(self.h, ptrs, ctypes_, len(types), kc, kd, len(key_columns), n, n if lead is None else lead,
                                               perm.ctypes.data, C.addressof(ties), C.addressof(bits), C.addressof(words)))
        return perm[:n], ties.value, list(bits), words.value

    def prim_gather_tuples(self, tuples, tuple_size: int, perm, n_out: int) -> np.ndarray:
        """out tuple i = tuple perm[i] for i < n_out on the device (rsq_prim_gather_tuples): tuples uint8 [n_rows * tuple_size]; returns
        the device's buffer as uint8 [n_out * tuple_size + 64] - the gathered tuples and, behind them, 64 guard bytes that are still
        0xEE where the kernel kept to its range"""
        tuples = np.ascontiguousarray(tuples).view(np.uint8).reshape(-1)
        perm = np.ascontiguousarray(perm, dtype=np.uint32)
        n = len(tuples) // tuple_size
        out = np.zeros(n_out * tuple_size + 64, dtype=np.uint8)
        self._check(self._L.rsq_prim_gather_tuples(self.h, tuples.ctypes.data, tuple_size, n, perm.ctypes.data, n_out, out.ctypes.data, len(out)))
        return out

    def set_order_sort(self, where: int):
        """where an ORDER BY over a materialisation is sorted: 0 the host's quicksort over all tuples (the default), 1 the device orders
        the rows by their keys and delivers the tuples (rsq_ctx_set_order_sort).  Read at every execution; Query.order_sort_report says
        which path ran and why"""
        self._check(self._L.rsq_ctx_set_order_sort(self.h, where))

    def set_result_pack(self, where: int):
        """where a materialisation's result tuples are packed: 0 on the host from columns copied one by one (the default), 1 on the
        device, copied once (rsq_ctx_set_result_pack).  Read at every execution; Query.result_pack_report says which path ran and why"""
        self._check(self._L.rsq_ctx_set_result_pack(self.h, where))

    def set_order_limit(self, where: int):
        """where an ORDER BY ... LIMIT k over a materialisation is decided: 0 the host sorts every row (the default), 1 from candidates
        the device selects (rsq_ctx_set_order_limit).  Read at every execution; Query.order_limit_report says which path ran and why"""
        self._check(self._L.rsq_ctx_set_order_limit(self.h, where))

    def set_result_text(self, where: int):
        """where results become text under mode 0 and the statement loop's `tofile`: 0 on the host (the default), 1 on the device
        (rsq_ctx_set_result_text)"""
        self._check(self._L.rsq_ctx_set_result_text(self.h, where))

    def set_row_cells(self, mode: int):
        """the register aggregation's second form, rows into per-lane LDS cells: -1 chosen by the executions' kernel times (the default),
        0 not generated for statements compiled from now on, 1 in every launch that fits it (rsq_ctx_set_row_cells)"""
        self._check(self._L.rsq_ctx_set_row_cells(self.h, mode))

    def set_rowstore_bridge(self, where: int):
        """where row stores are transposed under mode 0 (and so by rsq_table_from_rowstore): 0 on the host (the default), 1 on the
        device (rsq_ctx_set_rowstore_bridge)"""
        self._check(self._L.rsq_ctx_set_rowstore_bridge(self.h, where))

    def set_stream(self, hip_stream: Optional[int]):
        """launch on the caller's HIP stream (an integer handle, 0 = the null stream; e.g.
        torch.cuda.current_stream().cuda_stream), or None to go back to the context's own stream"""
        self._check(self._L.rsq_ctx_set_stream(self.h, hip_stream or None, 0 if hip_stream is None else 1))

    def _adopt(self, child):
        """queries, tables and databases hold device memory of this context: they are closed before it is destroyed"""
        import weakref
        if not hasattr(self, "_children"):
            self._children = weakref.WeakSet()
        self._children.add(child)

    def close(self):
        if getattr(self, "h", None):
            for child in list(getattr(self, "_children", ())):
                try:
                    child.close()
                except Exception:
                    pass
            if not getattr(self, "_borrowed", False):
                self._L.rsq_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tables ----
    def table(self, t: P.Table) -> "DeviceTable":
        keep: list = []
        d = t.to_c(keep)
        h = C.c_void_p()
        self._check(self._L.rsq_table_create(self.h, C.byref(d), C.byref(h)))
        return DeviceTable(self, h, t.name, {c.name: c.type.width for c in t.columns})

    def table_from_device(self, name: str, n_rows: int, columns) -> "DeviceTable":
        """columns: list of (name, SqlType, device_pointer_or_None); pointers stay owned by the caller"""
        cols = (P.rsq_column * len(columns))()
        for i, (cn, ct, ptr) in enumerate(columns):
            cols[i].name = cn.encode(); cols[i].type = ct.c(); cols[i].data = ptr
        d = P.rsq_table_desc(); d.name = name.encode(); d.n_rows = n_rows; d.n_cols = len(columns); d.cols = cols
        h = C.c_void_p()
        self._check(self._L.rsq_table_create_device(self.h, C.byref(d), C.byref(h)))
        return DeviceTable(self, h, name, {cn: ct.width for cn, ct, _ in columns})

    def load_tbl(self, schema: P.Table, path: str, terminator: str = "|", threads: int = 0, mode: int = 0, chunk_bytes: int = 0,
                 max_device_text_bytes: int = 0) -> "DeviceTable":
        """BULK INSERT of a '.tbl' text file into a table with `schema`'s column names and types (rsq_table_load_tbl_ex).  mode 0: parsed
        where the context's tbl_ingest says, TBL_HOST, TBL_DEVICE; the table's load_report says which path ran, why, and its phases"""
        keep: list = []
        bare = P.Table(schema.name, [P.Column(c.name, c.type) for c in schema.columns], 0)
        d = bare.to_c(keep)
        h = C.c_void_p()
        opt = rsq_tbl_load_options(C.sizeof(rsq_tbl_load_options), mode, chunk_bytes, max_device_text_bytes)
        rep = rsq_tbl_load_report(C.sizeof(rsq_tbl_load_report))
        self._check(self._L.rsq_table_load_tbl_ex(self.h, C.byref(d), path.encode(), terminator.encode()[:1], threads, C.byref(opt), C.byref(rep),
                                                  C.byref(h)))
        t = DeviceTable(self, h, schema.name, {c.name: c.type.width for c in schema.columns})
        t.load_report = rep.as_dict()
        return t

    def from_rowstore(self, schema: P.Table, blocks: Sequence, mode: int = 0, chunk_bytes: int = 0) -> "DeviceTable":
        """a table with `schema`'s column names and types out of a ReSQL row store (rsq_table_from_rowstore_ex): `blocks` are byte
        buffers (bytes, memoryviews, uint8 arrays - views at any offset) of packed tuples.  mode 0: transposed where the context's
        set_rowstore_bridge says, ROWSTORE_HOST, ROWSTORE_DEVICE; the table's bridge_report says which path ran, why, and its phases"""
        keep: list = []
        bare = P.Table(schema.name, [P.Column(c.name, c.type) for c in schema.columns], 0)
        d = bare.to_c(keep)
        views = [np.frombuffer(b, dtype=np.uint8) for b in blocks]
        ptrs = (C.c_void_p * max(1, len(views)))(*[v.ctypes.data for v in views])
        sizes = (C.c_size_t * max(1, len(views)))(*[v.size for v in views])
        h = C.c_void_p()
        opt = rsq_rowstore_options(C.sizeof(rsq_rowstore_options), mode, chunk_bytes)
        rep = rsq_rowstore_report(C.sizeof(rsq_rowstore_report))
        self._check(self._L.rsq_table_from_rowstore_ex(self.h, C.byref(d), ptrs, sizes, len(views), C.byref(opt), C.byref(rep), C.byref(h)))
        t = DeviceTable(self, h, schema.name, {c.name: c.type.width for c in schema.columns})
        t.bridge_report = rep.as_dict()
        return t

    def generate(self, kind: int, n_rows: int, sf: float, row0: int = 0, param: int = 0,
                 seed: int = 20240613) -> "DeviceTable":
        h = C.c_void_p()
        self._check(self._L.rsq_table_generate(self.h, kind, row0, n_rows, sf, param, seed, C.byref(h)))
        return DeviceTable(self, h, ["lineitem", "orders", "customer", "t"][kind])

    # ---- queries ----
    def compile(self, plan: P.Plan, tables: Sequence["DeviceTable"]) -> "Query":
        keep: list = []
        d = plan.to_c(keep)
        arr = (C.c_void_p * max(1, len(tables)))(*[t.h for t in tables])
        h = C.c_void_p()
        self._check(self._L.rsq_query_compile(self.h, C.byref(d), arr, len(tables), C.byref(h)))
        return Query(self, h)

    def run(self, plan: P.Plan, tables: Optional[Sequence["DeviceTable"]] = None) -> P.Result:
        """upload plan.tables (unless device tables are given), compile, execute, fetch the result"""
        own = tables is None
        tabs = [self.table(t) for t in plan.tables] if own else list(tables)
        try:
            q = self.compile(plan, tabs)
            try:
                q.execute()
                return q.result()
            finally:
                q.close()
        finally:
            if own:
                for t in tabs:
                    t.close()

    def serialize_expr(self, plan: P.Plan, expr: int, derive: bool, tables: Sequence["DeviceTable"] = ()) -> str:
        keep: list = []
        d = plan.to_c(keep)
        arr = (C.c_void_p * max(1, len(tables)))(*[t.h for t in tables])
        p = self._L.rsq_serialize_expr(self.h, C.byref(d), expr, 1 if derive else 0, arr, len(tables))
        if not p:
            raise EngineError(2, self._L.rsq_last_error(self.h).decode())
        s = C.string_at(p).decode("latin1")
        self._L.rsq_free(p)
        return s

    # ---- SQL text (the reference's parseSql + buildQuery in front of the path) ----
    def sql_describe(self, sql: str, what: int = 1) -> str:
        """what=0: token names, what=1: the parsed statement (see resql_hip.h rsq_sql_describe)"""
        p = self._L.rsq_sql_describe(self.h, sql.encode("latin1"), what)
        if not p:
            raise EngineError(2, self._L.rsq_last_error(self.h).decode())
        s = C.string_at(p).decode("latin1")
        self._L.rsq_free(p)
        return s

    def sql_plan(self, sql: str, tables: Sequence["DeviceTable"], host_tables: Sequence[P.Table] = ()) -> P.Plan:
        """plan of a select statement over the database `tables`, as a P.Plan (scan operators name their table;
        `host_tables` — same order — become plan.tables so that the oracle / the reference harness can run it)"""
        arr = (C.c_void_p * max(1, len(tables)))(*[t.h for t in tables])
        h = C.c_void_p()
        self._check(self._L.rsq_sql_plan_select(self.h, sql.encode("latin1"), arr, len(tables), C.byref(h)))
        try:
            d = self._L.rsq_sql_plan_desc(h).contents
            return P.Plan.from_c(d, [t.name for t in tables], list(host_tables))
        finally:
            self._L.rsq_sql_plan_destroy(h)

    def sql_plan_text(self, sql: str, tables: Sequence["DeviceTable"]) -> str:
        arr = (C.c_void_p * max(1, len(tables)))(*[t.h for t in tables])
        h = C.c_void_p()
        self._check(self._L.rsq_sql_plan_select(self.h, sql.encode("latin1"), arr, len(tables), C.byref(h)))
        try:
            p = self._L.rsq_sql_plan_text(h)
            if not p:
                raise EngineError(2, "rsq_sql_plan_text failed")
            s = C.string_at(p).decode("latin1")
            self._L.rsq_free(p)
            return s
        finally:
            self._L.rsq_sql_plan_destroy(h)

    def sql_compile(self, sql: str, tables: Sequence["DeviceTable"]) -> "Query":
        arr = (C.c_void_p * max(1, len(tables)))(*[t.h for t in tables])
        h = C.c_void_p()
        self._check(self._L.rsq_sql_compile(self.h, sql.encode("latin1"), arr, len(tables), C.byref(h)))
        return Query(self, h)

    def read_bandwidth(self, nbytes: int = 8 << 30, iters: int = 5) -> float:
        v = C.c_double()
        self._check(self._L.rsq_measure_read_bandwidth(self.h, nbytes, iters, C.byref(v)))
        return v.value


class DeviceTable:
    def __init__(self, ctx: Context, h, name: str, widths: Optional[dict] = None):
        self.ctx, self.h, self.name = ctx, h, name
        self.widths = dict(widths or {})          # bytes per row of the columns, by name, where the schema came through Python (read_image)
        self.load_report: Optional[dict] = None   # of Context.load_tbl
        self.bridge_report: Optional[dict] = None   # of Context.from_rowstore
        ctx._adopt(self)

    @property
    def n_rows(self) -> int:
        return self.ctx._L.rsq_table_rows(self.h)

    def set_row0(self, row0: int):
        """this table is rows [row0, row0 + n_rows) of a larger one (a shard); before queries are compiled over it"""
        self.ctx._check(self.ctx._L.rsq_table_set_first_row(self.h, row0))

    def append(self, more: "DeviceTable"):
        """the rows of `more` go behind this table's rows (BULK INSERT appends); `more` is consumed"""
        self.ctx._check(self.ctx._L.rsq_table_append(self.h, more.h))
        more.h = None

    def refresh_stats(self):
        """gather the column statistics again (adopted columns whose content changed); compile statements anew afterwards"""
        self.ctx._check(self.ctx._L.rsq_table_refresh_stats(self.h))

    @property
    def total_rows(self) -> int:
        """rows of the whole table this one is a shard of (its own count before unify_shard_stats)"""
        return self.ctx._L.rsq_table_total_rows(self.h)

    def stats_blob(self) -> bytes:
        """this shard's column statistics + row range as a fixed-size blob (the same size on every shard of a schema)"""
        n = self.ctx._L.rsq_table_stats_bytes(self.h)
        buf = C.create_string_buffer(n)
        self.ctx._check(self.ctx._L.rsq_table_stats_export(self.h, buf, n))
        return buf.raw

    def unify_shard_stats(self, blobs: Sequence[bytes]):
        """plan this shard as the whole table: `blobs` = stats_blob() of ALL shards (this one's included).  Before compiling."""
        joined = b"".join(blobs)
        self.ctx._check(self.ctx._L.rsq_table_unify_shard_stats(self.h, joined, len(blobs), len(blobs[0]) if blobs else 0))

    def time_dictionary_pass(self, name: str, which: int) -> float:
        """device ms of one pass over a coded column: which 0 the recode pass (identity map), 1 encoding the wide column anew; the codes stay"""
        ms = C.c_double(0)
        self.ctx._check(self.ctx._L.rsq_table_time_dictionary_pass(self.h, name.encode(), which, C.byref(ms)))
        return ms.value

    def read_column(self, name: str, dtype, count: Optional[int] = None) -> np.ndarray:
        n = self.n_rows if count is None else count
        out = np.empty(n, dtype=dtype)
        self.ctx._check(self.ctx._L.rsq_table_read_column(self.ctx.h, self.h, name.encode(), out.ctypes.data, out.nbytes))
        return out

    def image_info(self, name: str) -> tuple:
        """(narrow image's width in bytes or 0, its base, dictionary entries or 0, rows) of a column (rsq_table_read_image)"""
        info = (C.c_int64 * 4)()
        self.ctx._check(self.ctx._L.rsq_table_read_image(self.ctx.h, self.h, name.encode(), 0, None, 0, info))
        return tuple(int(v) for v in info)

    def read_image(self, name: str, which: int) -> np.ndarray:
        """the whole of a column's narrow image (which 0), dictionary entries (1) or dictionary codes (2), as bytes; empty if there is none"""
        if which not in (0, 1, 2):
            raise ValueError("read_image: which is 0 (narrow image), 1 (dictionary entries) or 2 (dictionary codes)")
        width, _, entries, rows = self.image_info(name)
        if which == 1 and entries and name not in self.widths:
            raise KeyError(f"read_image: the width of column {name} is not known to this handle")
        n = (rows * width, entries * self.widths.get(name, 0), rows if entries else 0)[which]
        out = np.empty(n, dtype=np.uint8)
        if n:
            info = (C.c_int64 * 4)()
            self.ctx._check(self.ctx._L.rsq_table_read_image(self.ctx.h, self.h, name.encode(), which, out.ctypes.data, n, info))
        return out

    def close(self):
        if self.h:
            self.ctx._L.rsq_table_destroy(self.h)
            self.h = None


class Query:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h
        ctx._adopt(self)

    def execute(self):
        self.ctx._check(self.ctx._L.rsq_query_execute(self.h))

    def await_kernels(self):
        """block until the query runs on its specialised kernels (it may have started on the pre-compiled generic pipeline)"""
        self.ctx._check(self.ctx._L.rsq_query_await_kernels(self.h))

    def execute_partial(self):
        """returns (device_pointer, n_min_words, n_max_words, n_sum_words)"""
        p = C.c_void_p(); a = C.c_int64(); b = C.c_int64(); c = C.c_int64()
        self.ctx._check(self.ctx._L.rsq_query_execute_partial(self.h, C.byref(p), C.byref(a), C.byref(b), C.byref(c)))
        return p.value, a.value, b.value, c.value

    def execute_partial_async(self):
        """enqueue the pipelines on the context's stream and return; finalize() synchronises (see resql_hip.h)"""
        self.ctx._check(self.ctx._L.rsq_query_execute_partial_async(self.h))

    def finalize_host(self, words: np.ndarray):
        """finalise from a partial aggregate table held in host memory (int64 words)"""
        w = np.ascontiguousarray(words, dtype=np.int64)
        self.ctx._check(self.ctx._L.rsq_query_finalize_host(self.h, w.ctypes.data_as(C.POINTER(C.c_int64)), w.size))

    def bind_partial(self, dev_ptr: int, nbytes: int):
        self.ctx._check(self.ctx._L.rsq_query_bind_partial(self.h, dev_ptr, nbytes))

    def merge_gathered(self, gathered_dev_ptr: int, n_ranks: int):
        """reduce the gathered partial tables of n_ranks ranks (device memory, back to back) into the bound partial table"""
        self.ctx._check(self.ctx._L.rsq_query_merge_gathered(self.h, gathered_dev_ptr, n_ranks))

    def partial_layout(self):
        """(n_min_words, n_max_words, n_sum_words) of the partial aggregate table"""
        a = C.c_int64(); b = C.c_int64(); c = C.c_int64()
        self.ctx._check(self.ctx._L.rsq_query_partial_layout(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def finalize(self):
        self.ctx._check(self.ctx._L.rsq_query_finalize(self.h))

    def result(self, text: bool = True) -> P.Result:
        """text=False skips the (pure Python) serialisation — for results with millions of rows"""
        v = P.rsq_result_view()
        self.ctx._check(self.ctx._L.rsq_query_result(self.h, C.byref(v)))
        res = P.Result.from_view(v)
        res.text = res.serialize() if text else None
        return res

    def result_text(self, mode: int = 0, chunk_rows: int = 0, max_device_bytes: int = 0):
        """(the result's '.tbl' text as bytes, the report as a dict) - rsq_query_result_text.  mode 0: written where the context's
        set_result_text says, TEXT_HOST, TEXT_DEVICE; the report says which path ran, why, rows, chunks and the phases"""
        opt = rsq_result_text_options(C.sizeof(rsq_result_text_options), mode, chunk_rows, max_device_bytes)
        rep = rsq_result_text_report(C.sizeof(rsq_result_text_report))
        p, n = C.c_void_p(), C.c_int64(0)
        self.ctx._check(self.ctx._L.rsq_query_result_text(self.h, C.byref(opt), C.byref(rep), C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value), rep.as_dict()
        finally:
            self.ctx._L.rsq_free(p)

    def write_result_text(self, path: str, mode: int = 0, chunk_rows: int = 0, max_device_bytes: int = 0) -> dict:
        """the same text straight into the file `path` (rsq_query_result_write); returns the report"""
        opt = rsq_result_text_options(C.sizeof(rsq_result_text_options), mode, chunk_rows, max_device_bytes)
        rep = rsq_result_text_report(C.sizeof(rsq_result_text_report))
        self.ctx._check(self.ctx._L.rsq_query_result_write(self.h, path.encode(), C.byref(opt), C.byref(rep)))
        return rep.as_dict()

    def report(self) -> rsq_report:
        r = rsq_report()
        self.ctx._check(self.ctx._L.rsq_query_report(self.h, C.byref(r)))
        return r

    def order_limit_report(self) -> dict:
        """rsq_order_limit_report: whether the plan is an ORDER BY ... LIMIT the device can pre-select for, and for the last execution
        which path decided the answer, why, rows, candidates and the phases"""
        return _report_of(self.ctx, rsq_order_limit_report, "rsq_query_order_limit_report", self.h)

    def order_sort_report(self) -> dict:
        """rsq_order_sort_report: whether the plan is an ORDER BY the device can sort, and for the last execution which side sorted,
        why, the composite key's bits, words and passes, the rows, the tied pairs and the phases"""
        return _report_of(self.ctx, rsq_order_sort_report, "rsq_query_order_sort_report", self.h)

    def result_pack_report(self) -> dict:
        """rsq_result_pack_report: whether the plan is a materialisation the device can pack, and for the last execution which side
        packed the result tuples, why, whether the host sorted them, the relation's size and the phases"""
        return _report_of(self.ctx, rsq_result_pack_report, "rsq_query_result_pack_report", self.h)

    def kernel_time_stats(self, reset: bool = False):
        """(device ms summed over the executions since the last reset, number of executions)"""
        s, n = C.c_double(0), C.c_uint64(0)
        self.ctx._check(self.ctx._L.rsq_query_kernel_time_stats(self.h, C.byref(s), C.byref(n), 1 if reset else 0))
        return s.value, n.value

    def nested_loops_slices(self) -> int:
        """S of the most recent execution's top nested-loops pipeline: the slices its launch cut the inner rows into (1: not split;
        0: no such join in the plan, or not executed yet)"""
        s = C.c_int32(0)
        self.ctx._check(self.ctx._L.rsq_query_nested_loops_slices(self.h, C.byref(s)))
        return s.value

    @property
    def source(self) -> str:
        return self.ctx._L.rsq_query_source(self.h).decode()

    @property
    def explain(self) -> str:
        return self.ctx._L.rsq_query_explain(self.h).decode()

    def close(self):
        if self.h:
            self.ctx._L.rsq_query_destroy(self.h)
            self.h = None


class Database:
    """The statement loop of the reference's executeStatement (execute.h:508-545) over the engine — the C ABI's rsq_db_*:
    CREATE TABLE records a schema, BULK INSERT loads a '.tbl' file into device columns, SELECT is parsed, planned, compiled
    and executed.  execute_script splits at ';' like expandExecStatements (execute.h:470-505)."""

    KINDS = {1: "SELECT", 2: "CREATE_TABLE", 3: "BULK_INSERT", 4: "CONTROL"}

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx._L.rsq_db_create(ctx.h, C.byref(h)))
        self.h = h
        ctx._adopt(self)

    def add_table(self, t: "DeviceTable"):
        """hand a device table to the database (which owns it from now on)"""
        self.ctx._check(self.ctx._L.rsq_db_adopt_table(self.h, t.h))
        t.h = None

    def execute(self, sql: str):
        """returns a P.Result for a select, None otherwise"""
        kind = C.c_int32(0)
        v = P.rsq_result_view()
        self.ctx._check(self.ctx._L.rsq_db_execute(self.h, sql.encode("latin1"), C.byref(kind), C.byref(v)))
        self.last_kind = self.KINDS.get(kind.value)
        if kind.value != 1:
            return None
        res = P.Result.from_view(v)
        res.text = res.serialize()
        return res

    @property
    def message(self) -> str:
        """what the reference's printQueryResult prints for the last statement in front of the relation"""
        return self.ctx._L.rsq_db_message(self.h).decode("utf8", "replace")

    def report(self) -> rsq_report:
        r = rsq_report()
        self.ctx._check(self.ctx._L.rsq_db_report(self.h, C.byref(r)))
        return r

    @property
    def load_report(self) -> dict:
        """rsq_tbl_load_report of the last BULK INSERT: which path parsed the file, why, rows, lines patched, phase times"""
        return _report_of(self.ctx, rsq_tbl_load_report, "rsq_db_load_report", self.h)

    @property
    def result_text_report(self) -> dict:
        """rsq_result_text_report of the last SELECT that `tofile` wrote: which path wrote qres.tbl, why, rows, chunks, phase times"""
        return _report_of(self.ctx, rsq_result_text_report, "rsq_db_result_text_report", self.h)

    @property
    def order_limit_report(self) -> dict:
        """rsq_order_limit_report of the last SELECT: which path decided its ORDER BY ... LIMIT, why, rows, candidates, phase times"""
        return _report_of(self.ctx, rsq_order_limit_report, "rsq_db_order_limit_report", self.h)

    def order_sort_report(self) -> dict:
        """rsq_order_sort_report of the last SELECT: which side sorted its ORDER BY, why, the composite key, the rows, phase times"""
        return _report_of(self.ctx, rsq_order_sort_report, "rsq_db_order_sort_report", self.h)

    def result_pack_report(self) -> dict:
        """rsq_result_pack_report of the last SELECT: which side packed its result tuples, why, the relation's size, phase times"""
        return _report_of(self.ctx, rsq_result_pack_report, "rsq_db_result_pack_report", self.h)

    def execute_script(self, text: str):
        res = None
        for stmt in text.split(";"):
            if stmt.strip():
                res = self.execute(stmt.strip())
        return res

    def close(self):
        if getattr(self, "h", None):
            self.ctx._L.rsq_db_destroy(self.h)
            self.h = None


class MultiContext:
    """one host process, N GPUs (include/resql_hip.h rsq_multi_*): shard contexts + the RCCL (or peer-copy) group-by merge"""

    def __init__(self, devices: Sequence[int], merge: int = MERGE_AUTO, cache_dir: Optional[str] = None, emission_order: int = 0,
                 compat_flags: int = 0, engine_flags: int = 0, nested_loops_max_pairs: int = 0, nested_loops_inner_slices: int = 0):
        """engine_flags, nested_loops_max_pairs, nested_loops_inner_slices: as for Context, on every shard (ENGINE_DERIVED_MULTI, for these handles only, runs derived
        aggregations across the shards; ENGINE_DICT_MULTI, likewise, gives the shards of a table one dictionary per coded column, so that a
        GROUP BY over it merges as dense partial tables; ENGINE_NESTED_LOOPS splits a nested-loops join's pairs
        by its outer side's rows; the budget bounds the whole statement's pairs)"""
        self._L = lib()
        self._devs = (C.c_int32 * len(devices))(*devices)
        self._cache = cache_dir.encode() if cache_dir else None
        self._base = rsq_config.make(0, self._cache, False, emission_order, compat_flags, engine_flags,
                                     nested_loops_max_pairs=nested_loops_max_pairs, nested_loops_inner_slices=nested_loops_inner_slices)
        cfg = rsq_multi_config(C.sizeof(rsq_multi_config), len(devices), C.pointer(self._base), self._devs, merge, 0)
        h = C.c_void_p()
        rc = self._L.rsq_multi_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise EngineError(rc, self._L.rsq_multi_last_error(None).decode())
        self.h = h
        self.n = len(devices)
        self.shards = [Context.borrowed(self._L.rsq_multi_ctx(h, i), devices[i]) for i in range(self.n)]

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(rc, self._L.rsq_multi_last_error(self.h).decode())

    @property
    def merge_name(self) -> str:
        return self._L.rsq_multi_merge_name(self.h).decode()

    def shard_rows(self, n_total: int, shard: int):
        a, b = C.c_int64(), C.c_int64()
        self._L.rsq_multi_shard_rows(n_total, self.n, shard, C.byref(a), C.byref(b))
        return a.value, b.value

    def generate(self, kind: int, n_rows_total: int, sf: float, param: int = 0, seed: int = 20240613) -> List["DeviceTable"]:
        arr = (C.c_void_p * self.n)()
        self._check(self._L.rsq_multi_table_generate(self.h, kind, n_rows_total, sf, param, seed, arr))
        name = ["lineitem", "orders", "customer", "t"][kind]
        return [DeviceTable(self.shards[i], C.c_void_p(arr[i]), name) for i in range(self.n)]

    def generate_on_key(self, kind: int, n_rows_total: int, sf: float, key_column: str, param: int = 0,
                        seed: int = 20240613) -> List["DeviceTable"]:
        """like generate, with every shard boundary moved to the next change of `key_column`"""
        arr = (C.c_void_p * self.n)()
        self._check(self._L.rsq_multi_table_generate_on_key(self.h, kind, n_rows_total, sf, param, seed, key_column.encode(), arr))
        name = ["lineitem", "orders", "customer", "t"][kind]
        return [DeviceTable(self.shards[i], C.c_void_p(arr[i]), name) for i in range(self.n)]

    def compile(self, plan: P.Plan, tables_per_shard: Sequence[Sequence["DeviceTable"]]) -> "MultiQuery":
        keep: list = []
        d = plan.to_c(keep)
        nt = len(tables_per_shard[0])
        flat = [t.h for shard in tables_per_shard for t in shard]
        arr = (C.c_void_p * max(1, len(flat)))(*flat)
        h = C.c_void_p()
        self._check(self._L.rsq_multi_query_compile(self.h, C.byref(d), arr, nt, C.byref(h)))
        return MultiQuery(self, h)

    def _adopt(self, query):
        import weakref
        if not hasattr(self, "_queries"):
            self._queries = weakref.WeakSet()
        self._queries.add(query)

    def close(self):
        """queries first (rsq_multi_query_destroy frees device memory of the shard contexts and reads their tables), then the
        shards' tables, then the handle (which deletes the contexts)"""
        if getattr(self, "h", None):
            for q in list(getattr(self, "_queries", ())):
                q.close()
            for s in self.shards:
                s.close()
            self._L.rsq_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiQuery:
    def __init__(self, m: MultiContext, h):
        self.m, self.h = m, h
        m._adopt(self)

    def execute(self):
        self.m._check(self.m._L.rsq_multi_query_execute(self.h))

    def result(self) -> P.Result:
        v = P.rsq_result_view()
        self.m._check(self.m._L.rsq_multi_query_result(self.h, C.byref(v)))
        res = P.Result.from_view(v)
        res.text = res.serialize()
        return res

    @property
    def merge_name(self) -> str:
        return self.m._L.rsq_multi_query_merge_name(self.h).decode()

    def explain(self, shard: int = 0) -> str:
        """the explain text of one shard's statement"""
        s = self.m._L.rsq_multi_query_explain(self.h, shard)
        if s is None:
            raise IndexError(f"no shard {shard}")
        return s.decode()

    @property
    def collective_ms(self) -> float:
        """device time of the last execution's group-by merge (event pair on the root's stream)"""
        return self.m._L.rsq_multi_query_collective_ms(self.h)

    def report(self):
        """(rsq_report, [kernel ms of every shard])"""
        r = rsq_report()
        k = (C.c_double * self.m.n)()
        self.m._check(self.m._L.rsq_multi_query_report(self.h, C.byref(r), k))
        return r, list(k)

    def close(self):
        if self.h:
            self.m._L.rsq_multi_query_destroy(self.h)
            self.h = None
